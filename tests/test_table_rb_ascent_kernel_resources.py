"""Register budget of the table RB-ascent kernels (csrc/d2d_tabascent.hip), read from the compiler's own metadata as
test_table_evaluate_kernel_resources.py reads the table what-if kernel's (no GPU needed: hipcc cross-compiles gfx950).  Only the
metadata fields are read; the instructions are nobody's business here.

Three kernels: the conversion in two instantiations, by the entry type of the table (float, double), and the ascent.  No scratch, no
spills - of vector or of scalar registers - no AGPRs; all launched with at most 256 threads, one wave per SIMD and workgroup, so four
workgroups per CU need at most 512 / 4 = 128 VGPRs per lane.  The conversion's LDS is static (one 32 x 33 tile and four flag words),
the ascent's one dynamic block.

The figures of the build this was written on: the ascent 54 VGPRs and 97 SGPRs; the conversion 72 VGPRs for both entry types, 48
(float) and 54 (double) SGPRs."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_tabascent.hip'
FIELDS = ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'group_segment_fixed_size', 'agpr_count',
          'max_flat_workgroup_size', 'vgpr_count', 'sgpr_count')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    from gym_d2d_amd import build
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not Path(hipcc).exists():
        pytest.skip('hipcc missing')
    tmp = tmp_path_factory.mktemp('isa_tabascent')
    cmd = [hipcc, *build.flags_for('d2d_tabascent.hip'), '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'tabascent.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    found = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+\S*?(tabgain_kernelI[fd]E|tabascent_kernel)', blk)
        if name:
            found[name.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)) for k in FIELDS}
    return found


def test_all_kernels_use_no_scratch_spill_nothing_and_stay_within_four_workgroups_per_cu(kernels):
    print(kernels)
    assert sorted(kernels) == ['tabascent_kernel', 'tabgain_kernelIdE', 'tabgain_kernelIfE']
    src = SOURCE.read_text()
    assert int(re.search(r'constexpr int TA_MAX_THREADS = (\d+);', src).group(1)) == 256
    assert int(re.search(r'constexpr int CV_THREADS = (\d+);', src).group(1)) == 256
    assert src.count('__launch_bounds__(TA_MAX_THREADS)') == 1 and src.count('__launch_bounds__(CV_THREADS)') == 1
    for name, k in kernels.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0, (name, k)
        assert k['max_flat_workgroup_size'] == 256, (name, k)
        assert k['vgpr_count'] <= 128, (name, k)
    assert kernels['tabascent_kernel']['group_segment_fixed_size'] == 0      # one dynamic block, carved by the host's offsets
    for name in ('tabgain_kernelIdE', 'tabgain_kernelIfE'):
        assert kernels[name]['group_segment_fixed_size'] == 32 * 33 * 4 + 16, (name, kernels[name])
