"""Build every shared library of `LIBRARIES`, `SOLVERS`, `ADDONS`, `FAMILIES`, `EXTRAS`, `EXACT`, `GROWING` and `LATER` for gfx950 with hipcc - in-tree, so the .so files travel with the repo snapshot.

    stem      libd2d_<stem>.so                                        public header
    hip       the product: the C ABI                                  include/d2d_hip.h
    probe     measurement equipment: the write-ceiling probe          include/d2d_hip_diag.h
    the rest  one stateless add-on kernel family each   include/d2d_<stem>.h
    assign    the RB matching, listed in SOLVERS        include/d2d_assign.h
    assignpwr the joint RB and power weights (4.17), listed in ADDONS   include/d2d_assignpwr.h
    color     the conflict-graph RB colouring (4.18), listed in ADDONS   include/d2d_color.h
    balance   the max-min SINR balancing (4.19), listed in FAMILIES      include/d2d_balance.h
    stable    the stable RB matching with quotas (4.20), listed in EXTRAS include/d2d_stable.h
    share     the exact optimal RB sharing (4.21), listed in EXACT        include/d2d_share.h
    ascent    the sum-capacity power ascent (4.22), listed in GROWING    include/d2d_ascent.h
    rbascent  the sum-capacity RB ascent (4.23), listed in LATER         include/d2d_rbascent.h
    goodput   the queue-aware goodput ascent (4.24), listed in LATER      include/d2d_goodput.h
    deviate   the unilateral-deviation gains (4.25), listed in LATER      include/d2d_deviate.h
    tabmarg   the difference rewards on a path-loss table (4.28), in LATER include/d2d_tabmarg.h
    evaltab   the what-if evaluation on a path-loss table (4.26), in LATER include/d2d_evaltab.h
    tabascent the sum-capacity RB ascent on a path-loss table (4.27), in LATER include/d2d_tabascent.h

    python -m gym_d2d_amd.build [--force] [--verbose]
    D2D_BUILD_DIAG=1 python -m gym_d2d_amd.build      # diagnostic build of libd2d_hip.so: the A/B tuning keys and the ablation
                                                      # switch of include/d2d_hip_diag.h are accepted (tools/ab_step.py ...)
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / 'csrc'
LIB_DIR = PKG / 'lib'
INCLUDE = PKG.parent / 'include'
ARCH = 'gfx950'

SOURCES = ['d2d_step.hip', 'd2d_rollout.hip', 'd2d_obs.hip', 'd2d_reset.hip', 'd2d_gain.hip', 'd2d_plan.hip', 'd2d_capi.hip']
# library stem -> its sources, in build order: the one table the digest, the up-to-date test, the compile and the link iterate
LIBRARIES = {'hip': SOURCES, 'probe': ['d2d_probe.hip', 'd2d_devfn.hip'],
             **{stem: [f'd2d_{stem}.hip'] for stem in ('plugin', 'episode', 'sense', 'graph', 'marginal', 'mobility', 'channel', 'queue',
                                                       'bestrb', 'powerctl', 'brdyn', 'evaluate')}}
# libraries that are no add-on kernel family of the table above (which _native.SIDE mirrors entry for entry): built and stamped
# with the rest, and a missing one is rebuilt (solvers_built()).  assign: the matching solver takes ANY weights, not only an env's
SOLVERS = {'assign': ['d2d_assign.hip']}
BUILT = {**LIBRARIES, **SOLVERS}
# further stateless kernel families (which _native.ADDONS mirrors): built and stamped with the rest, and a missing one is rebuilt
# (addons_built() for the row the table opened with, addons_missing() for every row).  Its two rows are fixed, as the tables above
# are: what joins the build now joins FAMILIES below.
# assignpwr: the joint RB and power weights; color: the conflict-graph RB colouring (4.18)
ADDONS = {'assignpwr': ['d2d_assignpwr.hip'], 'color': ['d2d_color.hip']}
EVERYTHING = {**BUILT, **ADDONS}                 # what build() compiles and links first, in order
# the stateless kernel families that joined since (which _native.FAMILIES mirrors): compiled and linked behind EVERYTHING, stamped with
# the rest, and a missing one is rebuilt (families_missing()).  This table is the one that grows.
# balance: the max-min SINR balancing
FAMILIES = {'balance': ['d2d_balance.hip']}
TARGETS = {**EVERYTHING, **FAMILIES}             # EVERYTHING and the families: fixed with them, as the tables above are
# the libraries that joined behind the families (which _native.EXTRAS mirrors): compiled and linked last, stamped with the rest, and a
# missing one is rebuilt (extras_missing()).
# stable: the stable RB matching with quotas
EXTRAS = {'stable': ['d2d_stable.hip']}
ALL = {**TARGETS, **EXTRAS}                      # TARGETS and the extras: fixed with them, as the tables above are
# the libraries that joined behind the extras (which _native.EXACT mirrors): compiled and linked last, stamped with the rest, and a
# missing one is rebuilt (exact_missing()).
# share: the exact optimal RB sharing for small link groups
EXACT = {'share': ['d2d_share.hip']}
WHOLE = {**ALL, **EXACT}                         # ALL and the exact solvers: fixed with them, as the tables above are
# the libraries that joined behind WHOLE (which _native.GROWING mirrors): compiled and linked last, stamped with the rest, and a
# missing one is rebuilt (growing_missing()).  Its one row is fixed, as the tables above are (tests/test_ascent_cpu.py states
# it): what joins the build now joins LATER below.
# ascent: the sum-capacity power ascent with SINR floors
GROWING = {'ascent': ['d2d_ascent.hip']}
EVERY = {**WHOLE, **GROWING}                     # WHOLE and what joined behind it: fixed with them, as the tables above are
# the libraries that joined behind EVERY (which _native.LATER mirrors): compiled and linked last, stamped with the rest, and a
# missing one is rebuilt (later_missing()).  The next library joins this table: nothing states its length.
# rbascent: the sum-capacity RB ascent with SINR floors; goodput: the queue-aware goodput ascent (4.24);
# deviate: the unilateral-deviation gains over every (RB, power) action (4.25); evaltab: the what-if evaluation on a path-loss table
# (4.26); tabascent: the sum-capacity RB ascent on a path-loss table (4.27); tabmarg: the difference rewards on a path-loss table
# (4.28), between deviate and evaltab - all four in front of goodput, which stays the build's last row
# (tests/test_goodput_ascent_cpu.py states it)
LATER = {'rbascent': ['d2d_rbascent.hip'], 'deviate': ['d2d_deviate.hip'], 'tabmarg': ['d2d_tabmarg.hip'],
         'evaltab': ['d2d_evaltab.hip'], 'tabascent': ['d2d_tabascent.hip'], 'goodput': ['d2d_goodput.hip']}
COMPLETE = {**EVERY, **LATER}                    # every library of the build: what the digest, the compile and the link iterate
HEADERS = [CSRC / 'd2d_internal.h', CSRC / 'd2d_plan.h', CSRC / 'd2d_step_device.h', CSRC / 'd2d_store.h', CSRC / 'd2d_same_rb.h', CSRC / 'd2d_addon.h',
           CSRC / 'd2d_powerctl_device.h', CSRC / 'd2d_wave_key.h', INCLUDE / 'd2d_hip.h', INCLUDE / 'd2d_hip_diag.h',
           *(INCLUDE / f'd2d_{stem}.h' for stem in TARGETS if stem not in ('hip', 'probe')),
           *(INCLUDE / f'd2d_{stem}.h' for stem in EXTRAS), *(INCLUDE / f'd2d_{stem}.h' for stem in EXACT),
           *(INCLUDE / f'd2d_{stem}.h' for stem in GROWING), *(INCLUDE / f'd2d_{stem}.h' for stem in LATER)]


def lib_path(stem: str, lib_dir: Path = LIB_DIR) -> Path:
    return lib_dir / f'libd2d_{stem}.so'


LIB_PATH = lib_path('hip')
PROBE_PATH = lib_path('probe')
STAMP = 'libd2d_hip.sha256'
FLAGS = ['-O3', '-std=c++17', '-fPIC', f'--offload-arch={ARCH}', '-fno-gpu-rdc', '-Wall', '-Wno-unused-function', '-Wno-unused-value',
         # the kernels already issue their uniform-address LDS atomics from one lane (or on rare paths): LLVM's atomic optimizer
         # only wraps them in mbcnt / readlane / popcount-multiply sequences
         '-mllvm', '-amdgpu-atomic-optimizer-strategy=None']
FLAGS += os.environ.get('D2D_BUILD_DEFINES', '').split()       # experiment builds (tools/ab_builds.py), e.g. -DD2D_EXP_PF_POS=1
if os.environ.get('D2D_BUILD_DIAG') == '1':          # diagnostic build: the step kernel honours D2D_TUNE_STEP_ABLATE
    FLAGS += ['-DD2D_DIAG=1', '-DD2D_STEP_ABLATE=1']
# flags of ONE source, appended behind FLAGS (every other source compiles as before, register for register).  d2d_obs.hip: the flat
# LinearObs kernels take scalar arguments so that the command processor preloads them into user SGPRs at wave launch (at most 14
# dwords: 16 user SGPRs less the kernarg segment pointer); a kernel whose argument is a struct by value is not affected
SOURCE_FLAGS = {'d2d_obs.hip': ['-mllvm', '-amdgpu-kernarg-preload-count=14']}


def flags_for(source: str) -> list:
    """The compile flags of `source` (a name of csrc/): FLAGS, then its row of SOURCE_FLAGS."""
    return [*FLAGS, *SOURCE_FLAGS.get(Path(source).name, [])]


def _hipcc() -> str:
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError('hipcc not found: libd2d_hip.so cannot be built (there is no CPU fallback)')


def digest_files() -> list:
    """The files source_digest() hashes, in order: every library's sources, then the headers."""
    return [p for p in [CSRC / s for sources in COMPLETE.values() for s in sources] + HEADERS if p.exists()]


def source_digest() -> str:
    """sha256 over the kernel / C-ABI sources, headers and compile flags: identifies what a profile was taken on."""
    h = hashlib.sha256()
    for p in digest_files():
        h.update(p.name.encode()); h.update(p.read_bytes())
    h.update(' '.join(FLAGS).encode())
    for name in sorted(SOURCE_FLAGS):
        h.update(name.encode()); h.update(' '.join(SOURCE_FLAGS[name]).encode())
    return h.hexdigest()


def up_to_date(digest: str, lib_dir: Path = LIB_DIR) -> bool:
    """Every library the package loads (all but the probe) is there and the stamp holds `digest`."""
    stamp = lib_dir / STAMP
    return all(p.exists() for p in [lib_path(stem, lib_dir) for stem in LIBRARIES if stem != 'probe'] + [stamp]) \
        and stamp.read_text().strip() == digest


def solvers_built(lib_dir: Path = LIB_DIR) -> bool:
    """Every library of SOLVERS is there; they share the stamp up_to_date() tests."""
    return all(lib_path(stem, lib_dir).exists() for stem in SOLVERS)


def addons_built(lib_dir: Path = LIB_DIR) -> bool:
    """The library of the row ADDONS opened with, assignpwr, is there - what this predicate has answered since that library was the
    whole table, and what a directory that holds that library alone still answers.  The rows that joined since are answered by
    addons_missing(); build() asks both.  They share the stamp up_to_date() tests."""
    return lib_path(next(iter(ADDONS)), lib_dir).exists()


def addons_missing(lib_dir: Path = LIB_DIR) -> list:
    """The stems of ADDONS whose library is not there, in the table's order: a missing one is rebuilt."""
    return [stem for stem in ADDONS if not lib_path(stem, lib_dir).exists()]


def families_missing(lib_dir: Path = LIB_DIR) -> list:
    """The stems of FAMILIES whose library is not there, in the table's order: a missing one is rebuilt."""
    return [stem for stem in FAMILIES if not lib_path(stem, lib_dir).exists()]


def extras_missing(lib_dir: Path = LIB_DIR) -> list:
    """The stems of EXTRAS whose library is not there, in the table's order: a missing one is rebuilt."""
    return [stem for stem in EXTRAS if not lib_path(stem, lib_dir).exists()]


def exact_missing(lib_dir: Path = LIB_DIR) -> list:
    """The stems of EXACT whose library is not there, in the table's order: a missing one is rebuilt."""
    return [stem for stem in EXACT if not lib_path(stem, lib_dir).exists()]


def growing_missing(lib_dir: Path = LIB_DIR) -> list:
    """The stems of GROWING whose library is not there, in the table's order: a missing one is rebuilt."""
    return [stem for stem in GROWING if not lib_path(stem, lib_dir).exists()]


def later_missing(lib_dir: Path = LIB_DIR) -> list:
    """The stems of LATER whose library is not there, in the table's order: a missing one is rebuilt."""
    return [stem for stem in LATER if not lib_path(stem, lib_dir).exists()]


def build(force: bool = False, verbose: bool = False) -> Path:
    LIB_DIR.mkdir(exist_ok=True)
    digest = source_digest()
    if not force and up_to_date(digest) and solvers_built() and addons_built() and not addons_missing() and not families_missing() \
            and not extras_missing() and not exact_missing() and not growing_missing() and not later_missing():
        return LIB_PATH
    hipcc = _hipcc()
    obj_dir = LIB_DIR / 'obj'
    obj_dir.mkdir(exist_ok=True)
    procs = []
    for s in [s for sources in COMPLETE.values() for s in sources]:
        src = CSRC / s
        obj = obj_dir / (src.stem + '.o')
        cmd = [hipcc, *flags_for(s), '-I', str(INCLUDE), '-c', str(src), '-o', str(obj)]
        if verbose:
            print(' '.join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f'hipcc failed on {s}:\n{out}')
        if verbose and out.strip():
            print(out)
    for stem, sources in COMPLETE.items():
        objs = [str(obj_dir / (Path(s).stem + '.o')) for s in sources]
        cmd = [hipcc, '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', str(lib_path(stem)), *objs]
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stdout}')
    (LIB_DIR / STAMP).write_text(digest)
    return LIB_PATH


if __name__ == '__main__':
    path = build(force='--force' in sys.argv, verbose='--verbose' in sys.argv or '-v' in sys.argv)
    print(path)
