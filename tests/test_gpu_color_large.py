"""color_kernel (csrc/d2d_color.hip) near its stated limits, launched directly through _native: 1024 and 1025 links (32 row words
exactly, and 33 with a last word of one bit), up to 160 112 of the 163 840 bytes of LDS a workgroup can have, up to 1000 RBs (32
`allowed` words with an 8-bit tail, a second and a fourth trip of the `r = tid; r < R; r += 256` loops), forced turns and the
clearing of the tally past 256 RBs, nine envs, and a mask on a multiple of 32 RBs.

One yardstick, no tolerance, as in test_gpu_color.py: color_util.color_graph fed the same tensors, all four outputs compared for
equality under both `pack` values, every launch into guarded allocations whose guard words are checked.  solver_large_util's table
names the path every case forces; test_solver_large_cpu.py asserts on the restatement alone that it is reached, and the same
conditions are asserted here on what the kernel returned.

Measured on an MI355X: all four outputs equal under both `pack` values in all nine cases - conflicts 0 at 1025 links on 24 RBs,
85 at 1024 links on 33 RBs (160 112 bytes), 690 / 595 at 600 links on 70 RBs, 40 and 269 on K300 and K520 with every RB past 256
loaded; the highest chosen RB is 299 of 300, 256 of 257 and 999 of 1000 (CHANGELOG.md, "Tests: the matching and colouring kernels at
2048 links and wide masks")."""
import numpy as np
import pytest

import color_util as cu
import solver_large_util as slu
from test_gpu_color import _case, _check, _launch, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.mark.parametrize('key', list(slu.COLOR_CASES), ids=lambda s: 'x'.join(map(str, s)))
def test_synthetic_scores_near_the_limits_equal_the_restatement(key):
    b, n, r = key
    c = slu.color_case(*key)
    turn = cu.turn_takers(n, r, c.movable, c.allowed)
    got = {}
    for pack in (False, True):
        got[pack] = _launch(c, pack)
        want = slu.color_ref(b, n, r, pack)
        print(f'{key}, pack={pack}: {int(turn.sum())} of {n} links take a turn on {r} RBs; conflicts {want[1].tolist()}, rbs_used '
              f'{want[2].tolist()}, proper {want[3].tolist()}; highest chosen RB {int(got[pack][0][:, turn].max())}; LDS '
              f'{slu.COLOR_CASES[key][1]} bytes')
        _same(got[pack], want, f'{key}, pack={pack}')
        rb = got[pack][0]
        assert np.array_equal(rb[:, ~turn], c.rb[:, ~turn])              # background rows are copied through, -1, R and R + 5 too
        assert ((rb[:, turn] >= 0) & (rb[:, turn] < r)).all()
        if c.allowed is not None:
            for e in range(b):
                assert c.allowed[np.nonzero(turn)[0], rb[e, turn]].all()
    held = c.rb[:, ~turn]
    assert (held == -1).any() and (held == r).any() and (held == r + 5).any() or turn.all()
    slu.color_reaches(key, c, turn, got)


@pytest.mark.parametrize('pack', [False, True])
@pytest.mark.parametrize('m,r', list(slu.COMPLETE_CASES))
def test_complete_graphs_past_256_rbs_tally_and_clear_every_rb(m, r, pack):
    """Every turn past the r-th is forced: the tally is taken over all RBs, reduced, and cleared over more than 256 of them."""
    score, thr, rb = slu.complete_inputs(m)
    full = _check(_case(score, thr, rb, r), pack, f'K{m} on {r} RBs')
    load = np.bincount(full[0][0], minlength=r)
    assert load.max() - load.min() <= 1 and load[256:].all()
    assert int(full[1][0]) == sum(int(k) * (int(k) - 1) // 2 for k in load) == slu.COMPLETE_CASES[(m, r)][1]
    assert int(full[2][0]) == r and int(full[3][0]) == 0
