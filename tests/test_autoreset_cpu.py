"""CPU side of VecD2DEnv's per-env autoreset: libd2d_episode.so's C header and exports, the ABI 7 constants of d2d_hip.h, the per-env
action stream of envs/_rng.py, the library's argument checks, and the full reset kernel's code (compiler output, no GPU)."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
GOLDEN = ROOT / 'tests' / 'golden'


def test_episode_header_is_valid_c_and_cpp():
    for compiler, std in (('gcc', '-std=c99'), ('g++', '-std=c++17')):
        if shutil.which(compiler) is None:
            pytest.skip(f'{compiler} missing')
        r = subprocess.run([compiler, std, '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-x', 'c' if compiler == 'gcc' else 'c++',
                            str(ROOT / 'include' / 'd2d_episode.h')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_episode_library_exports_exactly_its_header():
    from gym_d2d_amd import _native
    _native.load_episode_library()
    header = (ROOT / 'include' / 'd2d_episode.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / 'libd2d_episode.so')], capture_output=True, text=True,
                        check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}
    assert exported == declared == {'d2d_episode_merge_actions', 'd2d_episode_advance', 'd2d_episode_last_error'}
    assert set(_native.EPISODE_SIGNATURES) == declared
    lib = _native.load_episode_library()
    for name in declared:
        assert getattr(lib, name).argtypes is not None or name.endswith('last_error')


def test_episode_library_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    with pytest.raises(_native.NativeError, match='episode_length'):
        _native.episode_advance(0, 0, 0, 0, 0, 0, 1, 4, 0)
    with pytest.raises(_native.NativeError, match='null device pointer'):
        _native.episode_advance(0, 0, 0, 0, 0, 0, 1, 4, 10)
    with pytest.raises(_native.NativeError, match='null device pointer'):
        _native.episode_merge_actions(0, 0, 0, 0, 0, 4, 3, 0, 1)
    with pytest.raises(_native.NativeError, match='>= 0'):
        _native.episode_merge_actions(0, 0, 0, 0, 0, -1, 3, 0, 1)
    _native.episode_merge_actions(0, 0, 0, 0, 0, 0, 3, 0, 1)        # nothing to do: no launch, no error
    _native.episode_advance(0, 0, 0, 0, 0, 0, 1, 0, 10)


def _header_define(text, name):
    m = re.search(r'#define %s\s+(\S+)' % name, text)
    return m.group(1)


def test_abi7_constants_match_the_binding():
    from gym_d2d_amd import _native
    header = (ROOT / 'include' / 'd2d_hip.h').read_text()
    assert int(_header_define(header, 'D2D_ABI_VERSION')) == _native.ABI_VERSION == 7
    enum = dict((k, int(v)) for k, v in re.findall(r'(D2D_BUF_\w+)\s*=\s*(\d+)', header))
    assert enum['D2D_BUF_RESET_PENDING'] == _native.BUF_RESET_PENDING == 15
    assert enum['D2D_BUF_EPISODE'] == _native.BUF_EPISODE == 16
    assert enum['D2D_BUF_COUNT'] == _native.BUF_COUNT == 17
    assert _header_define(header, 'D2D_EPISODE_PER_ENV') == '((uint64_t)-1)'
    assert _native.EPISODE_PER_ENV == (1 << 64) - 1
    assert _native.BUFFER_DTYPES[_native.BUF_RESET_PENDING] == np.int32
    assert _native.BUFFER_DTYPES[_native.BUF_EPISODE] == np.uint32
    lib = _native.load_library()
    assert lib.d2d_abi_version() == 7


def test_per_env_buffers_have_one_entry_per_env():
    from gym_d2d_amd import _native
    h = _native.Handle.__new__(_native.Handle)
    h.num_envs, h.num_links, h.num_devices, h.num_fixed = 12, 50, 101, 0
    assert h.buffer_shape(_native.BUF_RESET_PENDING) == (12,)
    assert h.buffer_shape(_native.BUF_EPISODE) == (12,)


@pytest.mark.parametrize('seed,first_env,num_cols', [(0, 0, 50), (1234, 77, 7), ((1 << 63) + 5, 4000, 1)])
def test_per_env_draw_equals_the_lockstep_draw_row_by_row(seed, first_env, num_cols):
    from gym_d2d_amd.envs import _rng
    rng = np.random.default_rng(seed % 1000)
    episodes = rng.integers(0, 1 << 32, size=9, dtype=np.uint64)
    episodes[:3] = [0, 1, 2]
    high = rng.integers(1, 5000, size=num_cols)
    got = _rng.uniform_ints_numpy_per_env(seed, episodes, first_env, num_cols, high)
    assert got.shape == (9, num_cols) and got.dtype == np.int32
    for b, e in enumerate(episodes):
        want = _rng.uniform_ints_numpy(seed, int(e), first_env, 9, num_cols, high)[b]
        np.testing.assert_array_equal(got[b], want)


def _kernel_isa(asm, name):
    """The instruction stream of one kernel in a -save-temps .s file: comments and directives dropped, block labels renumbered
    from the function's own index (which only says where in the file the kernel sits)."""
    start = asm.index(name + ':')
    end = asm.index('.Lfunc_end', start)
    out = []
    for ln in asm[start:end].splitlines()[1:]:
        ln = ln.split(';')[0].strip()
        if not ln or (ln.startswith('.') and not ln.startswith('.LBB')):
            continue
        out.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s+', ' ', ln)))
    return out


def test_full_reset_kernel_compiles_to_the_isa_it_had_before_the_masked_variant(tmp_path):
    """The per-env reset is a sibling kernel sharing the unit body: the full reset's code must not move
    (tests/golden/reset_kernel_isa_gfx950.txt is the kernel of ABI 6)."""
    from gym_d2d_amd import build
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not Path(hipcc).exists():
        pytest.skip('hipcc missing')
    cmd = [hipcc, *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_reset.hip'), '-save-temps', '-o', 'reset.o']
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp_path.glob('*gfx950*.s')).read_text()
    got = _kernel_isa(asm, '_ZN3d2d12reset_kernelENS_9ResetArgsE')
    want = (GOLDEN / 'reset_kernel_isa_gfx950.txt').read_text().splitlines()
    assert got == want
    assert '_ZN3d2d19reset_masked_kernelENS_9ResetArgsENS_10MaskedArgsE:' in asm
