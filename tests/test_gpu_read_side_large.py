"""The three read-side kernels past 256 links and 64 KiB of LDS, launched directly through _native: csrc/d2d_marginal.hip
(marginal_kernel), csrc/d2d_graph.hip (coupling_kernel, neighbors_kernel, neighbor_obs_kernel) and csrc/d2d_sense.hip (sense_kernel).

The yardsticks are the float64 references of read_side_util.py, which test_read_side_cpu.py ties to the oracle; the bar is the
project's 1e-5 (golden_util.rel_err: |d| <= 1e-5 max(|ref|, 1)) throughout.  The case tables of read_side_util.py name the path
every case forces.  Every launch writes into an arena with guard words on both sides of every plane, over sentinels that a kernel
which skipped a row would leave behind, and is followed by torch.cuda.synchronize().  Every test prints the rel_err it measured.

What is NOT compared here:
  - marginal: the kernel does not return the capacity plane, and the step kernel is not launched, so difference == capacity - harm
    cannot be checked bit for bit against the step's plane as test_gpu_marginal.py does.  Instead difference + harm is held to the
    reference capacity at the bar, and on every link that is alone on its RB or on no RB harm is 0.0 exactly and the difference is,
    bit for bit, what a second launch gives in which every link has an RB of its own (the capacity alone).
  - marginal: the two planes are compared on the links the bar can decide (read_side_util.leave_one_out_direct; the CPU test holds
    the others under 1 % per case - 0 for every seed used here).
  - sense: the own-RB column of the 2048 x 64 case is not compared with the step kernel's sinr_db, for the same reason.
  - neighbor_obs: the grid-stride loop's second trip needs more than 2^28 groups (a 4 GiB output) and stays untested."""
import numpy as np
import pytest

import neighbors_util as nbu
import read_side_util as rsu
from golden_util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

BAR = rsu.BAR
GUARD, PAD = 0x5AFEC0DE, 64
SENT = 0x7FC0BEEF                              # what every output word holds before a launch: a NaN no kernel here produces


def _dev():
    return torch.device('cuda', 0)


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_device_side = {}


def _inputs(c):
    """The case's planes on the device, uploaded once per case object: pos_x, pos_y, rb, pwr, tx, rx, cols, cap_cols."""
    key = id(c)
    if key not in _device_side:
        _device_side[key] = (c, [torch.as_tensor(np.ascontiguousarray(a), device=_dev()) for a in
                                 (c['pos'][..., 0], c['pos'][..., 1], c['rb'], c['pwr'], c['tx'], c['rx'], c['cols'], c['cap_cols'])])
    return _device_side[key][1]


@pytest.fixture(scope='module', autouse=True)
def _drop_device_side():
    yield
    _device_side.clear()


class Arena:
    """Output planes of the given sizes (32-bit words) between guard words, each plane starting `shift` words past a 16-byte boundary
    and holding SENT.  host() checks every guard word and returns the planes as uint32."""

    def __init__(self, sizes, shift=0):
        self.sizes, self.at = list(sizes), []
        o = PAD + shift
        for s in self.sizes:
            self.at.append(o)
            o += ((s + 3) & ~3) + PAD
        self.t = torch.full((o,), GUARD, dtype=torch.int32, device=_dev())
        for a, s in zip(self.at, self.sizes):
            self.t[a:a + s] = SENT
        assert all(self.ptr(k) % 16 == 4 * shift for k in range(len(self.sizes)))

    def ptr(self, k):
        return self.t.data_ptr() + 4 * self.at[k]

    def host(self):
        torch.cuda.synchronize()                                        # raises if the device faulted
        h = self.t.cpu().numpy().view(np.uint32)
        for lo, hi in zip([0] + [a + s for a, s in zip(self.at, self.sizes)], self.at + [h.size]):
            assert (h[lo:hi] == GUARD).all(), 'a guard word was overwritten'
        return [h[a:a + s].copy() for a, s in zip(self.at, self.sizes)]


def _written(*planes):
    for p in planes:
        assert (p != SENT).all(), f'{int((p == SENT).sum())} output words were never written'


# ------------------------------------------------------------------------------------------ marginal_kernel
def _marginal(c):
    """One d2d_marginal_capacity launch: (harm, difference) float32 [B, N]."""
    from gym_d2d_amd import _native
    t = _inputs(c)
    words = c['b'] * c['n']
    arena = Arena([words, words])
    _native.marginal_capacity(*(x.data_ptr() for x in t), c['kind'], c['pow_k'], c['b'], c['d'], c['n'], c['r'], arena.ptr(0), arena.ptr(1),
                              _stream())
    harm, diff = arena.host()
    _written(harm, diff)
    return harm.view(np.float32).reshape(c['b'], c['n']), diff.view(np.float32).reshape(c['b'], c['n'])


def _capacity_alone(c):
    """The difference plane of a launch in which every link has an RB of its own: its capacity with nobody else on the air."""
    own = rsu.with_rb(c, np.broadcast_to(np.arange(c['n'], dtype=np.int32), (c['b'], c['n'])), c['n'])
    harm, diff = _marginal(own)
    assert (harm == 0.0).all() and not np.signbit(harm).any()
    return diff


def _check_marginal(what, c, harm, diff, ref):
    ref_diff, ref_harm, ref_cap, decided = ref
    assert harm.shape == diff.shape == ref_harm.shape and np.isfinite(harm).all() and np.isfinite(diff).all()
    e_h, e_d = rel_err(harm[decided], ref_harm[decided]), rel_err(diff[decided], ref_diff[decided])
    e_c = rel_err(diff[decided].astype(np.float64) + harm[decided], ref_cap[decided])
    same = c['rb'][:, :, None] == c['rb'][:, None, :]
    alone = (same.sum(axis=2) == 1) | c['bad']
    print(f'{what}: harm rel_err {e_h:.3e}, difference rel_err {e_d:.3e}, difference + harm vs the capacity {e_c:.3e} over {int(decided.sum())} '
          f'of {decided.size} links; harm up to {ref_harm.max():.3f} Mbps; {alone.mean():.1%} alone on their RB or on none')
    assert (~decided).mean() <= 0.01
    assert e_h <= BAR
    assert e_d <= BAR
    assert e_c <= BAR
    assert (harm >= 0.0).all()
    assert alone.any() and (harm[alone] == 0.0).all() and not np.signbit(harm[alone]).any()
    assert np.array_equal(_bits(diff[alone]), _bits(_capacity_alone(c)[alone]))
    return max(e_h, e_d)


@pytest.mark.parametrize('n,r,law,b,cell', rsu.MARGINAL_CASES)
def test_marginal_planes_against_the_member_list_reference(n, r, law, b, cell):
    """read_side_util.MARGINAL_CASES says which path each case is there for."""
    c = rsu.make_case(n, r, law, b=b, cell_radius=cell)
    ref = rsu.marginal_ref(n, r, law, b, cell)
    harm, diff = _marginal(c)
    _check_marginal(f'marginal {n} links, {r} RBs, {law}, {b} envs, {cell:.0f} m', c, harm, diff, ref)
    ref_harm = ref[1]
    if n == 2048:                                                       # link indices with bit 10 set have answers of their own
        assert (ref_harm[:, 1024:] > 0.0).any() and (harm[:, 1024:][ref_harm[:, 1024:] > 1e-3] > 0.0).all()
    if r == 1:                                                          # 300-member sums: everybody on the RB harms somebody
        assert (ref_harm[~c['bad']] > 0.0).all() and (harm[~c['bad']][ref_harm[~c['bad']] > 1e-3] > 0.0).all()
    if b > 1:                                                           # the env stride: env 1 is not env 0
        assert not np.array_equal(harm[0], harm[1])


def test_marginal_relaunched_gives_the_same_bits():
    n, r, law, b, cell = rsu.MARGINAL_RELAUNCH
    c = rsu.make_case(n, r, law, b=b, cell_radius=cell)
    first, again = _marginal(c), _marginal(c)
    for x, y in zip(first, again):
        assert np.array_equal(_bits(x), _bits(y))


def test_marginal_on_4000_rbs_gives_the_harm_of_the_same_plane_on_8():
    """The 1000-link 'mixed' case with a 16 KiB start array (86 KiB of LDS): one rb plane, out of range values included, launched on 8
    and on 4000 RBs, gives the same bits - and the bits of the 8-RB case it was made from, where the same links stand together."""
    on8, on4000 = rsu.wide_r_case()
    base = _marginal(rsu.make_case(1000, 8, 'mixed'))
    got8, got4000 = _marginal(on8), _marginal(on4000)
    for x, y, z in zip(base, got8, got4000):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(y), _bits(z))
    _check_marginal(f'marginal 1000 links, {rsu.MARGINAL_WIDE_R} RBs, mixed', on4000, *got4000,
                    rsu.marginal_ref(1000, rsu.MARGINAL_WIDE_R, 'mixed', 2, 500.0))


# ------------------------------------------------------------------------------------------ coupling_kernel
def _coupling(c, shift=0):
    from gym_d2d_amd import _native
    t = _inputs(c)
    arena = Arena([c['b'] * c['n'] * c['n']], shift)
    _native.graph_coupling(t[0].data_ptr(), t[1].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), c['kind'], c['pow_k'],
                           c['b'], c['d'], c['n'], arena.ptr(0), _stream())
    out, = arena.host()
    _written(out)
    return out.view(np.float32).reshape(c['b'], c['n'], c['n'])


_dense = {}


def _coupling_of(n, law, b, downlink=False):
    """(case, float64 reference, the kernel's dense matrix) of a link count, launched once."""
    key = (n, law, b, downlink)
    if key not in _dense:
        c, ref = rsu.neighbor_case(n, law, b, downlink)
        _dense[key] = (c, ref, _coupling(c))
    return _dense[key]


@pytest.fixture(scope='module', autouse=True)
def _drop_dense():
    yield
    _dense.clear()


@pytest.mark.parametrize('n,law,b', rsu.COUPLING_CASES)
def test_coupling_every_entry_against_the_float64_pair_loss(n, law, b):
    """read_side_util.COUPLING_CASES says which path each case is there for."""
    c, ref, got = _coupling_of(n, law, b)
    assert got.shape == ref.shape == (b, n, n) and np.isfinite(got).all()
    e = rel_err(got, ref)
    print(f'coupling {n} links, {law}, {b} envs: rel_err {e:.3e} over {ref.size} entries, {ref.min():.1f} .. {ref.max():.1f} dB')
    assert e <= BAR
    assert np.array_equal(_bits(got), _bits(_coupling(c)))              # two calls, the same bits
    if n == 260:
        # a base 4 bytes past alignment takes the dword stores and the lane + 64 q column mapping: same bits, guards intact
        assert np.array_equal(_bits(got), _bits(_coupling(c, shift=1)))


# ------------------------------------------------------------------------------------------ neighbors_kernel
def _neighbors(c, k, env_mask=None):
    """One d2d_graph_neighbors launch: (idx int32, coupling_db float32) [B, N, k]; rows the kernel skipped hold SENT."""
    from gym_d2d_amd import _native
    t = _inputs(c)
    words = c['b'] * c['n'] * k
    arena = Arena([words, words])
    m = None if env_mask is None else torch.as_tensor(np.asarray(env_mask, dtype=np.uint8), device=_dev())
    _native.graph_neighbors(t[0].data_ptr(), t[1].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), c['kind'], c['pow_k'],
                            c['b'], c['d'], c['n'], k, 0 if m is None else m.data_ptr(), arena.ptr(0), arena.ptr(1), _stream())
    idx, cdb = arena.host()
    shape = (c['b'], c['n'], k)
    return idx.reshape(shape), cdb.reshape(shape)


@pytest.mark.parametrize('n,law,b,down', rsu.NEIGHBOR_CASES)
def test_neighbor_lists_against_the_ranked_reference(n, law, b, down):
    """read_side_util.NEIGHBOR_CASES says which path each case is there for."""
    c, ref, dense = _coupling_of(n, law, b, down)
    ref_idx64, vals64, _ = rsu.neighbor_ranked(n, law, b, down, max(rsu.KS))      # a shorter ranking is its prefix
    for k in rsu.KS:
        idx_u, cdb_u = _neighbors(c, k)
        _written(idx_u, cdb_u)
        idx, cdb = idx_u.view(np.int32), cdb_u.view(np.float32)
        nbu.check_sets(idx, n)
        left_out, ties = nbu.check_indices(idx, ref, k)
        ref_idx, vals = ref_idx64[:, :, :k], vals64[:, :, :k]
        e = rel_err(cdb, vals)
        high = float((ref_idx >= 1024).mean())
        print(f'neighbors {n} links, {law}, downlink {down}, k={k}: values rel_err {e:.3e}; indices equal on every comparable entry, '
              f'{left_out:.2%} left out as near ties, {ties:.1%} of the gaps exact ties, {high:.1%} of the entries name a link >= 1024')
        assert e <= BAR
        assert (cdb[:, :, 1:] <= cdb[:, :, :-1]).all()
        # the values are the dense matrix's own entries, bit for bit
        assert np.array_equal(_bits(np.take_along_axis(dense, idx.astype(np.int64), axis=2)), _bits(cdb))
        if down and k >= 8:
            assert ties > 0.2                                           # the ascending-j rule is exercised
        if n == 2048 and law == 'ld35':
            assert high > 0.25 and (idx >= 1024).mean() > 0.25


def test_neighbors_env_mask_leaves_the_skipped_env_as_it_was():
    n, law, b, down = rsu.NEIGHBOR_CASES[0]
    c, _, _ = _coupling_of(n, law, b, down)
    k = 8
    full_idx, full_cdb = _neighbors(c, k)
    for mask in ([1, 0], [0, 7]):
        idx, cdb = _neighbors(c, k, env_mask=mask)
        for e, on in enumerate(mask):
            if on:
                assert np.array_equal(idx[e], full_idx[e]) and np.array_equal(cdb[e], full_cdb[e])
            else:
                assert (idx[e] == SENT).all() and (cdb[e] == SENT).all()


def test_neighbors_shorter_list_is_a_prefix_at_2048_links():
    n, law, b, down = rsu.NEIGHBOR_CASES[3]
    assert n == 2048
    c, _, _ = _coupling_of(n, law, b, down)
    i7, v7 = _neighbors(c, 7)
    i8, v8 = _neighbors(c, 8)
    _written(i7, v7)
    assert np.array_equal(i7, i8[:, :, :7]) and np.array_equal(v7, v8[:, :, :7])


# ------------------------------------------------------------------------------------------ neighbor_obs_kernel
def test_neighbor_obs_is_the_exact_gather_at_2048_links_and_k_64():
    """The lists of the 2048-link case and random planes, from an aligned base and from one 4 bytes past alignment."""
    from gym_d2d_amd import _native
    n, law, b, down = rsu.NEIGHBOR_CASES[3]
    c, _, _ = _coupling_of(n, law, b, down)
    k = 64
    idx_u, cdb_u = _neighbors(c, k)
    idx, cdb = idx_u.view(np.int32), cdb_u.view(np.float32)
    rng = np.random.default_rng(2048)
    rb = rng.integers(0, 330, (b, n)).astype(np.int32)
    pwr = rng.integers(0, 24, (b, n)).astype(np.int32)
    sinr = rng.normal(0.0, 30.0, (b, n)).astype(np.float32)
    snr = rng.normal(20.0, 30.0, (b, n)).astype(np.float32)
    want = nbu.gather_obs(idx.astype(np.int64), cdb.astype(np.float64), rb, pwr, sinr, snr).astype(np.float32)
    t = [torch.as_tensor(a, device=_dev()) for a in (idx, cdb, rb, pwr, sinr, snr)]
    for shift in (0, 1):
        arena = Arena([b * n * 4 * (k + 1)], shift)
        _native.graph_neighbor_obs(*(x.data_ptr() for x in t), b, n, k, arena.ptr(0), _stream())
        out, = arena.host()
        _written(out)
        assert np.array_equal(out.view(np.float32).reshape(b, n, -1), want), f'base {4 * shift} bytes past alignment'
    assert (idx >= 1024).mean() > 0.25


# ------------------------------------------------------------------------------------------ sense_kernel
def _sense(c, what, shift=0):
    from gym_d2d_amd import _native
    t = _inputs(c)
    arena = Arena([c['b'] * c['n'] * c['r']], shift)
    _native.sense_rb(*(x.data_ptr() for x in t[:7]), c['kind'], c['pow_k'], c['b'], c['d'], c['n'], c['r'],
                     {'sinr_db': _native.SENSE_SINR_DB, 'interference_mw': _native.SENSE_INTERFERENCE_MW}[what], arena.ptr(0), _stream())
    out, = arena.host()
    _written(out)
    return out.view(np.float32).reshape(c['b'], c['n'], c['r'])


@pytest.mark.parametrize('n,r,law,b', rsu.SENSE_CASES)
def test_sense_both_planes_against_the_float64_per_rb_sums(n, r, law, b):
    """read_side_util.SENSE_CASES says which path each case is there for."""
    c = rsu.make_case(n, r, law, b=b)
    pl = rsu.pair_pl_db(c)
    ref_ix = rsu.interference_per_rb(c, pl)
    ref_sinr = rsu.sinr_per_rb(c, ref_ix, pl)
    ix, sinr = _sense(c, 'interference_mw'), _sense(c, 'sinr_db')
    empty = ref_ix == 0.0
    assert (ix[empty] == 0.0).all() and (ix[~empty] > 0.0).all()
    e_i = rel_err(10 * np.log10(ix[~empty].astype(np.float64)), 10 * np.log10(ref_ix[~empty]))
    e_s = rel_err(sinr, ref_sinr)
    print(f'sense {n} links, {r} RBs, {law}, {b} envs: interference_mw rel_err {e_i:.3e} in dB ({empty.mean():.1%} of the entries empty), '
          f'sinr_db rel_err {e_s:.3e} over {ref_sinr.size} entries')
    assert np.isfinite(sinr).all()
    assert e_i <= BAR
    assert e_s <= BAR
    if (n, r) == (259, 44):
        # out 4 bytes past alignment with R % 4 == 0: vec_ok is 0 and the ragged tile leaves in dword stores - same bits, guards intact
        assert np.array_equal(_bits(ix), _bits(_sense(c, 'interference_mw', shift=1)))
        assert np.array_equal(_bits(sinr), _bits(_sense(c, 'sinr_db', shift=1)))
    if b > 1:
        assert not np.array_equal(sinr[0], sinr[1])
