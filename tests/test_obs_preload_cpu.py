"""The flat LinearObs kernels without a GPU: d2d_obs.hip compiled as build.py compiles it (FLAGS + its row of SOURCE_FLAGS) gives
every flat kernel a preloaded kernel-argument prefix of at least the twelve dwords a wave needs first, and no scalar load behind the
compatibility prologue at the block sizes that are template constants; every other kernel of the file, whose argument is a struct
by value, preloads nothing.  (T is staged through registers: staging by LDS-DMA measured slower, profiles/NEGATIVE_RESULTS.md.)
The per-source flags stay out of FLAGS (other sources compile as before) and are part of source_digest()."""
import os
import re
import subprocess

import pytest

# build.FLAGS as it stood before the per-source table (an experiment or diagnostic build appends to it, from the environment)
PARENT_FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-fno-gpu-rdc', '-Wall', '-Wno-unused-function',
                '-Wno-unused-value', '-mllvm', '-amdgpu-atomic-optimizer-strategy=None']


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    """mangled name -> (kernarg preload length, body text) of every kernel of d2d_obs.hip's gfx950 assembly"""
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('obs_asm')
    cmd = [build._hipcc(), *build.flags_for('d2d_obs.hip'), '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_obs.hip'),
           '-save-temps', '-o', 'k.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for name, descriptor in re.findall(r'^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel', asm, flags=re.M | re.S):
        m = re.search(r'\.amdhsa_user_sgpr_kernarg_preload_length (\d+)', descriptor)
        body = re.search(rf'^{re.escape(name)}:.*?^\.Lfunc_end\d+:', asm, flags=re.M | re.S)
        assert body, name
        out[name] = (int(m.group(1)) if m else 0, body.group(0))
    return out


def _is_flat(name):
    return 'obs_expand_flat_' in name


def test_every_flat_kernel_preloads_its_arguments(kernels):
    flat = {k: v for k, v in kernels.items() if _is_flat(k)}
    # float32 and float64 x six store policies x block {1024, 512, any}
    assert len(flat) == 36, sorted(flat)
    for name, (preload, body) in flat.items():
        assert preload >= 12, (name, preload)
        assert 'global_load_dwordx4' in body and 'ds_write_b128' in body, name          # the 16-byte staging, through registers
        # behind the prologue for firmware that does not preload (it ends in the branch to the aligned body) nothing is fetched by
        # scalar loads where the block size is a constant; any other block reads blockDim
        behind = body.split('.p2align\t8', 1)[1]
        assert ('s_load_' in behind) == ('ELi0EEEv' in name), name


def test_no_other_kernel_of_the_file_preloads(kernels):
    rest = {k: v for k, v in kernels.items() if not _is_flat(k)}
    assert rest and all('ObsArgs' in k for k in rest), sorted(rest)           # the row-aligned and the direct kernels keep the struct
    for name, (preload, body) in rest.items():
        assert preload == 0, (name, preload)


def test_the_flag_is_per_source_and_hashed(monkeypatch):
    from gym_d2d_amd import build
    assert build.FLAGS[:len(PARENT_FLAGS)] == PARENT_FLAGS
    if not os.environ.get('D2D_BUILD_DEFINES') and os.environ.get('D2D_BUILD_DIAG') != '1':
        assert build.FLAGS == PARENT_FLAGS
    assert not any('preload' in f for f in build.FLAGS)
    assert any('kernarg-preload-count' in f for f in build.SOURCE_FLAGS['d2d_obs.hip'])
    assert build.flags_for('d2d_obs.hip') == build.FLAGS + build.SOURCE_FLAGS['d2d_obs.hip']
    assert build.flags_for('d2d_step.hip') == build.FLAGS
    before = build.source_digest()
    monkeypatch.setattr(build, 'SOURCE_FLAGS', {'d2d_obs.hip': ['-mllvm', '-amdgpu-kernarg-preload-count=8']})
    changed = build.source_digest()
    monkeypatch.setattr(build, 'SOURCE_FLAGS', {})
    assert len({before, changed, build.source_digest()}) == 3
