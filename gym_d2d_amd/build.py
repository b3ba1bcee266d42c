"""Build libd2d_hip.so (the product: the C ABI of include/d2d_hip.h), libd2d_plugin.so (the stateless helpers of
include/d2d_plugin.h behind ArrayPathLoss's view.normal()), libd2d_episode.so (the stateless autoreset kernels of
include/d2d_episode.h), libd2d_sense.so (the stateless per-RB sensing kernel of include/d2d_sense.h), libd2d_graph.so (the stateless interference-graph kernels of
include/d2d_graph.h), libd2d_marginal.so (the stateless difference-reward kernel of include/d2d_marginal.h), libd2d_mobility.so (the stateless
Gauss-Markov move kernel of include/d2d_mobility.h), libd2d_channel.so (the stateless spatial-channel fill of
include/d2d_channel.h), libd2d_queue.so (the stateless packet-queue step of
include/d2d_queue.h), libd2d_bestrb.so (the stateless best-response RB selection of
include/d2d_bestrb.h), libd2d_powerctl.so (the stateless target-SINR power control of
include/d2d_powerctl.h), libd2d_brdyn.so (the stateless sequential best-response dynamics of
include/d2d_brdyn.h), libd2d_evaluate.so (the stateless what-if evaluation of candidate joint actions of
include/d2d_evaluate.h) and libd2d_probe.so (measurement equipment: the write-ceiling probe
of include/d2d_hip_diag.h) for gfx950 with hipcc - in-tree, so the .so files travel with the repo snapshot.

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
LIB_PATH = LIB_DIR / 'libd2d_hip.so'
PROBE_PATH = LIB_DIR / 'libd2d_probe.so'
PLUGIN_PATH = LIB_DIR / 'libd2d_plugin.so'
EPISODE_PATH = LIB_DIR / 'libd2d_episode.so'
SENSE_PATH = LIB_DIR / 'libd2d_sense.so'
GRAPH_PATH = LIB_DIR / 'libd2d_graph.so'
MARGINAL_PATH = LIB_DIR / 'libd2d_marginal.so'
MOBILITY_PATH = LIB_DIR / 'libd2d_mobility.so'
CHANNEL_PATH = LIB_DIR / 'libd2d_channel.so'
QUEUE_PATH = LIB_DIR / 'libd2d_queue.so'
BESTRB_PATH = LIB_DIR / 'libd2d_bestrb.so'
POWERCTL_PATH = LIB_DIR / 'libd2d_powerctl.so'
BRDYN_PATH = LIB_DIR / 'libd2d_brdyn.so'
EVALUATE_PATH = LIB_DIR / 'libd2d_evaluate.so'
INCLUDE = PKG.parent / 'include'
ARCH = 'gfx950'

SOURCES = ['d2d_step.hip', 'd2d_rollout.hip', 'd2d_obs.hip', 'd2d_reset.hip', 'd2d_gain.hip', 'd2d_plan.hip', 'd2d_capi.hip']
PROBE_SOURCES = ['d2d_probe.hip']
PLUGIN_SOURCES = ['d2d_plugin.hip']
EPISODE_SOURCES = ['d2d_episode.hip']
SENSE_SOURCES = ['d2d_sense.hip']
GRAPH_SOURCES = ['d2d_graph.hip']
MARGINAL_SOURCES = ['d2d_marginal.hip']
MOBILITY_SOURCES = ['d2d_mobility.hip']
CHANNEL_SOURCES = ['d2d_channel.hip']
QUEUE_SOURCES = ['d2d_queue.hip']
BESTRB_SOURCES = ['d2d_bestrb.hip']
POWERCTL_SOURCES = ['d2d_powerctl.hip']
BRDYN_SOURCES = ['d2d_brdyn.hip']
EVALUATE_SOURCES = ['d2d_evaluate.hip']
HEADERS = [CSRC / 'd2d_internal.h', CSRC / 'd2d_plan.h', CSRC / 'd2d_step_device.h', CSRC / 'd2d_store.h', CSRC / 'd2d_same_rb.h', CSRC / 'd2d_addon.h', INCLUDE / 'd2d_hip.h', INCLUDE / 'd2d_hip_diag.h',
           INCLUDE / 'd2d_plugin.h', INCLUDE / 'd2d_episode.h', INCLUDE / 'd2d_sense.h', INCLUDE / 'd2d_graph.h', INCLUDE / 'd2d_marginal.h', INCLUDE / 'd2d_mobility.h', INCLUDE / 'd2d_channel.h', INCLUDE / 'd2d_queue.h', INCLUDE / 'd2d_bestrb.h', INCLUDE / 'd2d_powerctl.h', INCLUDE / 'd2d_brdyn.h', INCLUDE / 'd2d_evaluate.h']
FLAGS = ['-O3', '-std=c++17', '-fPIC', f'--offload-arch={ARCH}', '-fno-gpu-rdc', '-Wall', '-Wno-unused-function', '-Wno-unused-value',
         # the kernels already issue their uniform-address LDS atomics from one lane (or on rare paths): LLVM's atomic optimizer
         # only wraps them in mbcnt / readlane / popcount-multiply sequences
         '-mllvm', '-amdgpu-atomic-optimizer-strategy=None']
FLAGS += os.environ.get('D2D_BUILD_DEFINES', '').split()       # experiment builds (tools/ab_builds.py), e.g. -DD2D_EXP_PF_POS=1
if os.environ.get('D2D_BUILD_DIAG') == '1':          # diagnostic build: the step kernel honours D2D_TUNE_STEP_ABLATE
    FLAGS += ['-DD2D_DIAG=1', '-DD2D_STEP_ABLATE=1']


def _hipcc() -> str:
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError('hipcc not found: libd2d_hip.so cannot be built (there is no CPU fallback)')


def source_digest() -> str:
    """sha256 over the kernel / C-ABI sources, headers and compile flags: identifies what a profile was taken on."""
    h = hashlib.sha256()
    for p in [CSRC / s for s in SOURCES + PROBE_SOURCES + PLUGIN_SOURCES + EPISODE_SOURCES + SENSE_SOURCES + GRAPH_SOURCES + MARGINAL_SOURCES + MOBILITY_SOURCES + CHANNEL_SOURCES + QUEUE_SOURCES + BESTRB_SOURCES + POWERCTL_SOURCES + BRDYN_SOURCES + EVALUATE_SOURCES if (CSRC / s).exists()] + [h for h in HEADERS if h.exists()]:
        h.update(p.name.encode()); h.update(p.read_bytes())
    h.update(' '.join(FLAGS).encode())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = False) -> Path:
    LIB_DIR.mkdir(exist_ok=True)
    stamp = LIB_DIR / 'libd2d_hip.sha256'
    digest = source_digest()
    if not force and LIB_PATH.exists() and PLUGIN_PATH.exists() and EPISODE_PATH.exists() and SENSE_PATH.exists() and GRAPH_PATH.exists() and MARGINAL_PATH.exists() and MOBILITY_PATH.exists() and CHANNEL_PATH.exists() and QUEUE_PATH.exists() and BESTRB_PATH.exists() and POWERCTL_PATH.exists() and BRDYN_PATH.exists() and EVALUATE_PATH.exists() and stamp.exists() and stamp.read_text().strip() == digest:
        return LIB_PATH
    hipcc = _hipcc()
    obj_dir = LIB_DIR / 'obj'
    obj_dir.mkdir(exist_ok=True)
    procs = []
    for s in SOURCES + PROBE_SOURCES + PLUGIN_SOURCES + EPISODE_SOURCES + SENSE_SOURCES + GRAPH_SOURCES + MARGINAL_SOURCES + MOBILITY_SOURCES + CHANNEL_SOURCES + QUEUE_SOURCES + BESTRB_SOURCES + POWERCTL_SOURCES + BRDYN_SOURCES + EVALUATE_SOURCES:
        src = CSRC / s
        obj = obj_dir / (src.stem + '.o')
        cmd = [hipcc, *FLAGS, '-I', str(INCLUDE), '-c', str(src), '-o', str(obj)]
        if verbose:
            print(' '.join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f'hipcc failed on {s}:\n{out}')
        if verbose and out.strip():
            print(out)
    for lib, sources in ((LIB_PATH, SOURCES), (PROBE_PATH, PROBE_SOURCES), (PLUGIN_PATH, PLUGIN_SOURCES),
                         (EPISODE_PATH, EPISODE_SOURCES), (SENSE_PATH, SENSE_SOURCES), (GRAPH_PATH, GRAPH_SOURCES),
                         (MARGINAL_PATH, MARGINAL_SOURCES), (MOBILITY_PATH, MOBILITY_SOURCES), (CHANNEL_PATH, CHANNEL_SOURCES),
                         (QUEUE_PATH, QUEUE_SOURCES), (BESTRB_PATH, BESTRB_SOURCES),
                         (POWERCTL_PATH, POWERCTL_SOURCES), (BRDYN_PATH, BRDYN_SOURCES),
                         (EVALUATE_PATH, EVALUATE_SOURCES)):
        objs = [str(obj_dir / (Path(s).stem + '.o')) for s in sources]
        cmd = [hipcc, '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', str(lib), *objs]
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stdout}')
    stamp.write_text(digest)
    return LIB_PATH


if __name__ == '__main__':
    path = build(force='--force' in sys.argv, verbose='--verbose' in sys.argv or '-v' in sys.argv)
    print(path)
