"""Register budget of the goodput-ascent kernel (csrc/d2d_goodput.hip), read from the compiler's own metadata as
test_rb_ascent_kernel_resources.py reads the RB ascent's (no GPU needed: hipcc cross-compiles gfx950).  Only the metadata fields
are read; the instructions are nobody's business here.

Three instantiations (inverse square 0, the general power law 1, pow-k 4).  No scratch, no spills - of vector or of scalar
registers - and no static LDS in front of the dynamic block; launched with at most 256 threads, that is at most one wave per SIMD
and workgroup, so four waves per SIMD - four envs per CU - need at most 512 / 4 = 128 VGPRs per lane.  The source text holds no
`atomic`.

The figures of the build this was written on: 57, 59 and 57 VGPRs, 94, 96 and 101 SGPRs, no AGPRs.  (With one array per field
instead of one record per link, the result pointers held across the turn loop and a wave count kept for the two combines the
instantiations spilled 7, 12 and 16 scalar registers.)"""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_goodput.hip'
FIELDS = ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'group_segment_fixed_size', 'agpr_count',
          'max_flat_workgroup_size', 'vgpr_count', 'sgpr_count')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    from gym_d2d_amd import build
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not Path(hipcc).exists():
        pytest.skip('hipcc missing')
    tmp = tmp_path_factory.mktemp('isa_goodput')
    cmd = [hipcc, *build.flags_for('d2d_goodput.hip'), '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'goodput.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    found = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+\S*(goodput_kernelILi\d+E)', blk)
        if name:
            found[name.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)) for k in FIELDS}
    return found


def test_three_kernels_use_no_scratch_spill_nothing_and_stay_within_four_waves_per_simd(kernels):
    print(kernels)
    assert sorted(kernels) == ['goodput_kernelILi0E', 'goodput_kernelILi1E', 'goodput_kernelILi4E']
    src = SOURCE.read_text()
    threads = int(re.search(r'constexpr int GP_MAX_THREADS = (\d+);', src).group(1))
    assert threads == 256 and '__launch_bounds__(GP_MAX_THREADS)' in src and 'min(GP_MAX_THREADS, (list + 63) & ~63)' in src
    for name, k in kernels.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['group_segment_fixed_size'] == 0 and k['agpr_count'] == 0, (name, k)
        assert k['max_flat_workgroup_size'] == threads, (name, k)
        assert k['vgpr_count'] <= 128, (name, k)


def test_the_source_text_holds_no_atomic():
    assert 'atomic' not in SOURCE.read_text()
