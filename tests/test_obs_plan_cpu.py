"""The LinearObs expansion planner (plan_obs, gym_d2d_amd/csrc/d2d_plan.hip) without a GPU: launch shape and store policy of the
headline shape in float32 and float64, the policies set by hand, and the shapes that must stay on the kernels they had.
tests/c/obs_plan.cpp drives plan_obs, compiled with hipcc as host code."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ('block', 'pieces', 'chunks', 'policy', 'vec', 'variant')

# (id, configuration, block, pieces per workgroup (rows of the row-aligned kernel), chunks, store policy, floats per store, variant)
PLANS = [
    # 512 rows of 768 float4 = 393216 pieces in slabs of 2 x 1024: the geometry of rounds 4-6, written through since T is staged in one trip
    ('headline_float32', 'B=4096 N=512', 1024, 2, 192, 5, 4, 2),
    # 512 rows of 1536 double2 = 786432 pieces in slabs of 2 x 1024
    ('headline_float64', 'B=4096 N=512 f64=1', 1024, 2, 384, 5, 2, 2),
    ('policy_1_by_hand', 'B=4096 N=512 tune_nt=1', 1024, 2, 192, 1, 4, 2),
    ('policy_1_by_hand_float64', 'B=4096 N=512 f64=1 tune_nt=1', 1024, 2, 384, 1, 2, 2),
    ('policy_0_by_hand', 'B=4096 N=512 tune_nt=0', 1024, 2, 192, 0, 4, 2),
    ('policy_5_by_hand_row_aligned', 'B=4 N=131 tune_nt=5', 448, 2, 66, 5, 2, 0),
    ('block_by_hand_float64', 'B=4096 N=512 f64=1 tune_block=512', 512, 2, 768, 5, 2, 2),
    # three and four pieces: written through only when asked for
    ('pieces_3_block_512', 'B=8 N=512 tune_rows=3 tune_block=512', 512, 3, 256, 1, 4, 2),
    ('pieces_4_policy_5_by_hand', 'B=8 N=512 tune_rows=4 tune_nt=5', 1024, 4, 96, 5, 4, 2),
    ('pieces_1', 'B=8 N=512 tune_rows=1', 1024, 1, 384, 5, 4, 2),
    # odd N: 8-byte rows - the row-aligned kernel, nontemporal as before; float64: flat, T staged in 8-byte granules, 1024 x 2, nontemporal
    ('odd_n_row_aligned', 'B=4 N=131', 448, 2, 66, 1, 2, 0),
    ('odd_n_float64', 'B=4 N=131 f64=1', 1024, 2, 26, 1, 2, 2),
    ('smallest_flat', 'B=3 N=2', 1024, 2, 1, 5, 4, 2),
]


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    from gym_d2d_amd import build
    exe = tmp_path_factory.mktemp('obs_plan') / 'obs_plan'
    cmd = [build._hipcc(), '-O1', '-std=c++17', '-Wall', '-x', 'hip', '--offload-host-only', '-I', str(build.INCLUDE),
           str(build.CSRC / 'd2d_plan.hip'), str(ROOT / 'tests' / 'c' / 'obs_plan.cpp'), '-o', str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(configs):
        r = subprocess.run([str(exe), *configs], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return [json.loads(line) for line in r.stdout.splitlines()]
    return run


def test_obs_plans(plan):
    got = plan([case[1] for case in PLANS])
    assert len(got) == len(PLANS)
    for (name, _, *want), p in zip(PLANS, got):
        assert [p[k] for k in FIELDS] == want, (name, p)


def test_xcd_grouping_needs_whole_groups_of_eight_envs(plan):
    got = plan(['B=16 N=130', 'B=9 N=130', 'B=16 N=130 f64=1', 'B=9 N=130 f64=1'])
    assert [p['xcd_remap'] for p in got] == [1, 0, 1, 0]


def test_chunk_division_is_a_multiply_shift_only_where_it_is_exact(plan):
    """ObsArgs::chunk_magic = ceil(2^40 / chunks) for the flat kernels while (blocks [/ 8]) x chunks < 2^40 and blocks [/ 8] < 2^24;
    beyond that, and for the row-aligned kernels, 0: the kernel divides."""
    got = plan(['B=4096 N=512', 'B=4096 N=512 f64=1', 'B=9 N=130', 'B=1000000 N=512', 'B=4 N=131'])
    assert [p['chunk_magic'] for p in got] == [-(-(1 << 40) // 192), -(-(1 << 40) // 384), -(-(1 << 40) // p_chunks(130)), 0, 0]
    for p, blocks in ((got[0], 4096 * 192 // 8), (got[2], 9 * p_chunks(130))):          # exact at the ends of the range and around multiples
        d, m = p['chunks'], p['chunk_magic']
        for n in (0, 1, d - 1, d, d + 1, blocks // 2 * 1 + 1, blocks - d, blocks - d - 1, blocks - 1):
            assert (n * m) >> 40 == n // d, (n, d)


def p_chunks(n, block=1024, pieces=2):
    return -(-(n * 6 * n // 4) // (block * pieces))
