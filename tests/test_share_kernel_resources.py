"""Register budget of the exact RB sharing kernels (csrc/d2d_share.hip), read from the compiler's own metadata as
test_kernel_resources.py reads the step kernels' (no GPU needed: hipcc cross-compiles gfx950).

No scratch, no spills, no static LDS in front of the dynamic block; each kernel within the vector registers its __launch_bounds__
imply at full occupancy of its workgroup - 256 threads: 128 VGPRs keep four workgroups on a CU; 1024 threads: 128 VGPRs are all a
SIMD has for the four waves it takes of one workgroup - and no atomics of any kind: every output word has one owner.

The figures of the build this was written on: share_values_kernel 38 - 41 VGPRs (the three laws), share_solve_kernel 44."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_share.hip'
FIELDS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count', 'private_segment_fixed_size',
          'group_segment_fixed_size', 'max_flat_workgroup_size')


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    from gym_d2d_amd import build
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not Path(hipcc).exists():
        pytest.skip('hipcc missing')
    tmp = tmp_path_factory.mktemp('isa_share')
    cmd = [hipcc, *build.flags_for('d2d_share.hip'), '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'share.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    kernels = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+\S*(share_values_kernelILi\d+E|share_solve_kernel)', blk)
        if name:
            kernels[name.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)) for k in FIELDS}
    return asm, kernels


def test_both_kernels_use_no_scratch_and_stay_within_their_launch_bounds(report):
    asm, kernels = report
    print(kernels)
    assert sorted(kernels) == ['share_solve_kernel', 'share_values_kernelILi0E', 'share_values_kernelILi1E', 'share_values_kernelILi4E']
    for name, k in kernels.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['group_segment_fixed_size'] == 0 and k['agpr_count'] == 0, (name, k)
        assert k['max_flat_workgroup_size'] == (1024 if name == 'share_solve_kernel' else 256), (name, k)
        assert k['vgpr_count'] <= 128, (name, k)
    assert 'scratch_' not in asm


def test_no_atomics_of_any_kind(report):
    asm, _ = report
    assert not re.search(r'^\s*(global|flat|buffer)_\w*atomic', asm, flags=re.M)
    assert not re.search(r'^\s*ds_(\w*rtn\w*|add_\w+|sub_\w+|min_\w+|max_\w+|and_\w+|or_\w+|xor_\w+|cmpst_\w+|inc_\w+|dec_\w+|pk_add\w+)\s', asm, flags=re.M)
    code = SOURCE.read_text().split('#include', 1)[1]
    assert not re.findall(r'\batomic\w+', code)
