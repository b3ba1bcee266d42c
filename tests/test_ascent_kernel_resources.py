"""Register budget of the power-ascent kernel (csrc/d2d_ascent.hip), read from the compiler's own metadata as
test_share_kernel_resources.py reads the sharing kernels' (no GPU needed: hipcc cross-compiles gfx950).

Three instantiations (inverse square 0, the general power law 1, pow-k 4).  No scratch, no spills - of vector or of scalar
registers - and no static LDS in front of the dynamic block; launched with 256 threads, that is one wave per SIMD and workgroup, so
four waves per SIMD - four envs per CU - need at most 512 / 4 = 128 VGPRs per lane.  No atomics of any kind.

The figures of the build this was written on: 50, 54 and 56 VGPRs, 87, 93 and 100 SGPRs, no AGPRs."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_ascent.hip'
FIELDS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count', 'private_segment_fixed_size',
          'group_segment_fixed_size', 'max_flat_workgroup_size')


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    from gym_d2d_amd import build
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not Path(hipcc).exists():
        pytest.skip('hipcc missing')
    tmp = tmp_path_factory.mktemp('isa_ascent')
    cmd = [hipcc, *build.flags_for('d2d_ascent.hip'), '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'ascent.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    kernels = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+\S*(ascent_kernelILi\d+E)', blk)
        if name:
            kernels[name.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)) for k in FIELDS}
    return asm, kernels


def test_three_kernels_use_no_scratch_spill_nothing_and_stay_within_four_waves_per_simd(report):
    asm, kernels = report
    print(kernels)
    assert sorted(kernels) == ['ascent_kernelILi0E', 'ascent_kernelILi1E', 'ascent_kernelILi4E']
    src = SOURCE.read_text()
    threads = int(re.search(r'constexpr int AS_THREADS = (\d+);', src).group(1))
    assert threads == 256 and '__launch_bounds__(AS_THREADS)' in src and 'dim3(AS_THREADS)' in src
    for name, k in kernels.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['group_segment_fixed_size'] == 0 and k['agpr_count'] == 0, (name, k)
        assert k['max_flat_workgroup_size'] == threads, (name, k)
        assert k['vgpr_count'] <= 512 // 4, (name, k)
    assert 'scratch_' not in asm


def test_no_atomics_of_any_kind(report):
    asm, _ = report
    assert not re.search(r'^\s*(global|flat|buffer)_\w*atomic', asm, flags=re.M)
    assert not re.search(r'^\s*ds_(\w*rtn\w*|add_\w+|sub_\w+|min_\w+|max_\w+|and_\w+|or_\w+|xor_\w+|cmpst_\w+|inc_\w+|dec_\w+|pk_add\w+)\s', asm, flags=re.M)
    code = SOURCE.read_text().split('#include', 1)[1]
    assert not re.findall(r'\batomic\w+', code)
