"""Register budget of the table difference-reward kernel (csrc/d2d_tabmarg.hip), read from the compiler's own metadata as
test_table_evaluate_kernel_resources.py reads the table what-if kernel's (no GPU needed: hipcc cross-compiles gfx950).  Only the
metadata fields are read; the instructions are nobody's business here.

Two instantiations, by the entry type of the table (float, double).  No scratch, no spills - of vector or of scalar registers - no
AGPRs, no static LDS (one dynamic block, carved by the host's offsets); launched with 256 threads, one wave per SIMD and workgroup,
so four workgroups per CU need at most 512 / 4 = 128 VGPRs per lane.  DESIGN.md 4.28 records the counts of the build it was written
on."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_tabmarg.hip'
FIELDS = ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'group_segment_fixed_size', 'agpr_count',
          'max_flat_workgroup_size', 'vgpr_count', 'sgpr_count')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    from gym_d2d_amd import build
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not Path(hipcc).exists():
        pytest.skip('hipcc missing')
    tmp = tmp_path_factory.mktemp('isa_tabmarg')
    cmd = [hipcc, *build.flags_for('d2d_tabmarg.hip'), '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'tabmarg.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    found = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+\S*?(tabmarg_kernelI[fd]E)', blk)
        if name:
            found[name.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)) for k in FIELDS}
    return found


def test_both_instantiations_use_no_scratch_spill_nothing_and_stay_within_four_workgroups_per_cu(kernels):
    print(kernels)
    assert sorted(kernels) == ['tabmarg_kernelIdE', 'tabmarg_kernelIfE']
    src = SOURCE.read_text()
    assert int(re.search(r'constexpr int TM_THREADS = (\d+);', src).group(1)) == 256
    assert src.count('__launch_bounds__(TM_THREADS)') == 1
    for name, k in kernels.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['group_segment_fixed_size'] == 0, (name, k)
        assert k['max_flat_workgroup_size'] == 256, (name, k)
        assert k['vgpr_count'] <= 128, (name, k)
