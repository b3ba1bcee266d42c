"""Register budget of the deviation kernels (csrc/d2d_deviate.hip), read from the compiler's own metadata as
test_goodput_kernel_resources.py reads the goodput ascent's (no GPU needed: hipcc cross-compiles gfx950).  Only the metadata fields
are read; the instructions are nobody's business here.

Two kernels, the table and the best deviation, in three instantiations each (inverse square 0, the general power law 1, pow-k 4),
and the regret kernel behind the second.  No scratch, no spills - of vector or of scalar registers - no AGPRs; launched with at most
256 threads, that is at most one wave per SIMD and workgroup, so four workgroups per CU need at most 512 / 4 = 128 VGPRs per lane.
The source text holds no `atomic`.

The figures of the build this was written on: 56, 56 and 54 VGPRs for both kernels, 77 to 87 SGPRs; the regret kernel 22 and 42."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_deviate.hip'
FIELDS = ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'group_segment_fixed_size', 'agpr_count',
          'max_flat_workgroup_size', 'vgpr_count', 'sgpr_count')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    from gym_d2d_amd import build
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not Path(hipcc).exists():
        pytest.skip('hipcc missing')
    tmp = tmp_path_factory.mktemp('isa_deviate')
    cmd = [hipcc, *build.flags_for('d2d_deviate.hip'), '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'deviate.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    found = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+\S*(deviate_kernelILi\d+ELb[01]E|regret_kernel)', blk)
        if name:
            found[name.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)) for k in FIELDS}
    return found


def test_the_kernels_use_no_scratch_spill_nothing_and_stay_within_four_workgroups_per_cu(kernels):
    print(kernels)
    assert sorted(kernels) == sorted([f'deviate_kernelILi{mode}ELb{best}E' for mode in (0, 1, 4) for best in (0, 1)] + ['regret_kernel'])
    src = SOURCE.read_text()
    threads = int(re.search(r'constexpr int DV_MAX_THREADS = (\d+);', src).group(1))
    assert threads == 256 and src.count('__launch_bounds__(DV_MAX_THREADS)') == 2
    for name, k in kernels.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0, (name, k)
        assert k['max_flat_workgroup_size'] == threads, (name, k)
        assert k['vgpr_count'] <= 128, (name, k)
        if name != 'regret_kernel':                  # its flags and keys are static; the two big kernels carve one dynamic block
            assert k['group_segment_fixed_size'] == 0, (name, k)


def test_the_source_text_holds_no_atomic():
    assert 'atomic' not in SOURCE.read_text()
