"""step_kernel (csrc/d2d_step.hip) in its two path-loss table modes - PL_TABLE (gains converted once, by device pair or by link pair,
uploaded from the host or converted from device memory by gain_from_db_kernel) and PL_TABLE_DB (the caller's live [B][N+1][N] dB table,
float32 or float64, converted inside the step) - at every launch shape launch_step instantiates: the 36 kernels of
tests/table_route_util.py's case table, each by the Simulator shape and tuning keys test_table_route_cpu.py shows the planner to answer
with that kernel.  One test per (case, route group):

    host     R1 d2d_set_path_loss_table (a `devices` table, per-env and shared), R2 d2d_set_path_loss_link_table (its gather, and a
             `pairs` table, per-env and shared; 2.42 M entries at 1100 links: three upload chunks, the third behind its event)
    device   R3 d2d_set_path_loss_link_table_dev (f64 and f32 per-env, shared once; 2.42 M f64 entries at 1100 links and 4.19 M shared
             f32 entries at 2048 are past the conversion kernel's grid of num_cus x 32 x 256: its grid-stride loop goes round again),
             R4 the live table (f64 and f32, row N the diagonal and an SNR row of its own)

The tables are seeded draws per (env, tx, rx), not functions of a distance: not symmetric, no two entries of an env equal, two CUE
columns of a row different, unread device pairs NaN - [tx][rx] against [rx][tx], a receiver's column against its device, one env's
block against another's all change the result.  Every output plane (SINR, SNR, rate, capacity, reward, obs table, rb, pwr, env flags)
is bound to a guard_util.Guarded allocation and filled with a NaN pattern before each launch: afterwards the bands are intact and
every word is written.

Yardstick 1, bit equality on every plane: the interferer-search variants of sim_util within a route (where no tuning key fixes the
search), R1 on a device table = R2 on its gather, R3 = R4 at the same dtype with row N the diagonal, a shared table = the same
table repeated per env, a second launch = the first.  (Host and device conversions are not held bit-identical: pow and exp2 may differ
in the double's last bit.)  Yardstick 2, the float64 reference table_step_ref: |d| <= 1e-5 max(|ref|, 1) on sinr_db, snr_db, rate_bps,
capacity_mbps and the reward, links within 1e-4 dB of their sensitivity left out of rate and capacity and their envs out of the
reward; float32 tables are the float64 draws rounded once and the reference reads the rounded values.  Every case has an env with
out-of-range RBs, so no case's status word is 0: every other env's flag word is, and the status word is FLAG_RB_OUT_OF_RANGE alone.

Measured on an MI355X (256 CUs): the worst deviation of any case, route and plane 1.4e-6 of the bar's max(|ref|, 1) (sinr_db,
n130_lpt2_lists), per case in CHANGELOG.md; 51 tests in 7 s, none over 0.8 s.  The 2100-link row of the case table is planned only:
d2d_create takes 2048 links, and the strided kernel is launched at 2048 (n2048_strided)."""
import numpy as np
import pytest
import torch

import table_route_util as tr
from guard_util import Guarded
from sim_util import OUTS, assert_same, search_variants

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC0BEEF                  # a quiet NaN as float32, an impossible rb / pwr / flag word as int32
TUNE_KEYS = {'epw': 'TUNE_STEP_ENVS_PER_WG', 'lpt': 'TUNE_STEP_LPT', 'threads': 'TUNE_STEP_THREADS'}


class Rig:
    """A Simulator in the case's shape, its output planes bound to guarded allocations, one path-loss table installed at a time."""

    def __init__(self, native, case):
        from gym_d2d_amd.simulator import Simulator
        self.native, self.case = native, case
        self.sim = sim = Simulator(dict(num_rbs=case.rbs, num_cues=case.cues, num_due_pairs=case.dues, num_envs=case.b), max_links=case.n)
        self.h = h = sim.handle
        self.pos = tr.positions(case)
        sim.set_positions(self.pos)
        sim.set_links(sim.default_link_keys())
        tx, rx, ty = tr.links(case)
        assert np.array_equal(sim.link_tx, tx) and np.array_equal(sim.link_rx, rx) and np.array_equal(sim.link_type, ty)
        h.set_obs_mode(native.OBS_TABLE)
        h.set_reward(case.reward, tr.REWARD_PARAM[case.reward])
        for key, value in case.tune:
            h.set_tuning(getattr(native, TUNE_KEYS[key]), value)
        if case.walk is not None:
            h.set_tuning(native.TUNE_STEP_WALK, case.walk)
        h.set_bucketing(case.bucketing)
        self.act = tr.actions(case)
        if self.act.fixed is not None:
            h.set_fixed_actions(*self.act.fixed)
        self.planes = {}
        for name in OUTS:
            which = getattr(native, name)
            shape = h.buffer_shape(which)
            g = Guarded(shape, torch.int32 if native.BUFFER_DTYPES.get(which, np.float32) == np.int32 else torch.float32)
            h.bind_buffer(which, g.array.data_ptr(), g.nbytes)
            self.planes[name] = g
        self.inputs = ('BUF_RB', 'BUF_PWR') if case.stepping == 'planes' else ()
        if self.inputs:
            h.upload(native.BUF_RB, self.act.rb.astype(np.int32))
            h.upload(native.BUF_PWR, self.act.pwr.astype(np.int32))
        self.live = None                          # the live table, held while steps read it

    def close(self):
        self.h.synchronize()
        self.h.close()

    # ---- the routes
    def r1(self, dev_table):
        self.h.set_path_loss_table(dev_table)

    def r2(self, link_table):
        self.h.set_path_loss_link_table(link_table)

    def r3(self, link_table, dtype):
        t = torch.as_tensor(np.array(link_table, dtype=dtype), device='cuda')
        torch.cuda.synchronize()
        self.h.set_path_loss_link_table_dev(t.data_ptr(), self.native.F64 if dtype == np.float64 else self.native.F32, self.case.n,
                                            int(t.ndim == 3))

    def r4(self, link_table, snr, dtype):
        """[B, N+1, N]: link_table [B, N, N] above row N = snr [B, N] (None: the diagonal)."""
        row = np.diagonal(link_table, axis1=1, axis2=2) if snr is None else snr
        self.h.synchronize()                      # the last step may still read the table this one replaces
        self.live = torch.as_tensor(np.ascontiguousarray(np.concatenate([link_table, row[:, None, :]], axis=1), dtype=dtype), device='cuda')
        torch.cuda.synchronize()
        self.h.set_path_loss_link_table_dev(self.live.data_ptr(), self.native.F64 if dtype == np.float64 else self.native.F32,
                                            self.case.n, self.native.PL_TABLE_LIVE)

    # ---- one launch
    def launch(self):
        for name, g in self.planes.items():
            if name not in self.inputs:
                g.array.view(torch.int32).fill_(PATTERN)
        torch.cuda.synchronize()
        if self.case.stepping == 'planes':
            self.h.step_rb_pwr()
        else:
            self.sim.step_arrays(self.act.raw)
        self.h.synchronize()
        snap = {}
        for name, g in self.planes.items():
            assert g.intact(), (self.case.name, name)
            snap[name] = g.array.view(torch.int32).cpu().numpy().copy()
            assert (snap[name] != PATTERN).all(), (self.case.name, name, int((snap[name] == PATTERN).sum()))
        return snap

    def step(self):
        """Two launches (the same words) under every search variant the case leaves open (the same words); the snapshot."""
        def twice():
            first, second = self.launch(), self.launch()
            assert_same({'first': first, 'second': second}, 'first')
            return first
        if self.case.walk is None and self.case.bucketing:
            snaps = search_variants(self.native, self.h, twice)
            assert_same(snaps)
            return snaps['auto']
        return twice()

    # ---- yardstick 2
    def check(self, snap, pl, snr=None, tag=''):
        case, native = self.case, self.native
        ref = tr.reference(case, pl, snr)
        f = {name: snap[name].view(np.float32) for name in OUTS if name not in ('BUF_RB', 'BUF_PWR', 'BUF_ENV_FLAGS')}
        keep, keep_env = ~ref['near'], ~ref['near_env']
        errs = {'sinr_db': tr.rel_err(f['BUF_SINR_DB'], ref['sinr_db']), 'snr_db': tr.rel_err(f['BUF_SNR_DB'], ref['snr_db']),
                'rate_bps': tr.rel_err(f['BUF_RATE_BPS'], ref['rate_bps'], keep),
                'capacity_mbps': tr.rel_err(f['BUF_CAPACITY'], ref['capacity_mbps'], keep),
                'reward': tr.rel_err(f['BUF_REWARD'][keep_env], ref['reward'][keep_env])}
        print(f'{case.name} {tag}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= tr.TOL, (case.name, tag, k, v)
        # the obs table: the link's position row (float64 positions: their float32 roundings), then the SINR and SNR planes' words
        tx, rx, _ = tr.links(case)
        p32 = self.pos.astype(np.float32)
        table = snap['BUF_OBS_TABLE']
        assert np.array_equal(table[:, :, :2].view(np.float32), p32[:, tx]) and np.array_equal(table[:, :, 2:4].view(np.float32), p32[:, rx])
        assert np.array_equal(table[:, :, 4], snap['BUF_SINR_DB']) and np.array_equal(table[:, :, 5], snap['BUF_SNR_DB'])
        assert np.array_equal(snap['BUF_RB'], self.act.rb) and np.array_equal(snap['BUF_PWR'], self.act.pwr)
        want = np.zeros(case.b, dtype=np.int32)
        want[tr.special_envs(case)[1]] = native.FLAG_RB_OUT_OF_RANGE
        assert np.array_equal(snap['BUF_ENV_FLAGS'], want), (case.name, tag, snap['BUF_ENV_FLAGS'])
        assert self.h.status_flags() == native.FLAG_RB_OUT_OF_RANGE          # nothing else in any env: the out-of-range env's word alone


@pytest.fixture
def rig(native, request):
    rigs = []

    def make(name):
        rigs.append(Rig(native, tr.BY_NAME[name]))
        return rigs[-1]
    yield make
    for r in rigs:
        r.close()


def _repeated(t, b):
    return np.ascontiguousarray(np.broadcast_to(t[None], (b,) + t.shape))


def _rounded(t, dtype):
    """The table as the route holds it: the float64 draws, or their float32 roundings read back as float64."""
    return t if dtype == np.float64 else t.astype(np.float32).astype(np.float64)


SMALL = [c.name for c in tr.GPU_CASES if 'R1' in c.routes]
LARGE_HOST = [c.name for c in tr.GPU_CASES if 'R1' not in c.routes and 'R2' in c.routes]
LARGE_DEVICE = [c.name for c in tr.GPU_CASES if 'R1' not in c.routes]


@pytest.mark.parametrize('name', SMALL)
def test_host_routes(rig, name):
    """R1 and R2: a device table against its gather, a pairs table, each per-env and shared, against the reference."""
    r = rig(name)
    c = r.case
    for shared in (False, True):
        dev = tr.devices(c, shared)
        link = tr.gather(c, dev)
        r.r1(dev)
        a = r.step()
        r.check(a, link, tag=f'R1 shared={shared}')
        r.r2(link)
        assert_same({'R1': a, 'R2 on the gather': r.step()}, 'R1')
        if shared:
            r.r1(_repeated(dev, c.b))
            assert_same({'shared': a, 'repeated per env': r.step()}, 'shared')
        pairs = tr.pairs(c, shared)
        r.r2(pairs)
        a = r.step()
        r.check(a, pairs, tag=f'R2 shared={shared}')
        if shared:
            r.r2(_repeated(pairs, c.b))
            assert_same({'shared': a, 'repeated per env': r.step()}, 'shared')


@pytest.mark.parametrize('name', SMALL)
def test_device_routes(rig, name):
    """R3 and R4: the conversion kernel against the conversion inside the step (bit for bit), f64 and f32; the SNR's own row; a shared
    table once."""
    r = rig(name)
    c = r.case
    inp = tr.inputs(c.name)
    for dtype in (np.float64, np.float32):
        held = _rounded(inp.pairs, dtype)
        r.r3(inp.pairs, dtype)
        a = r.step()
        r.check(a, held, tag=f'R3 {np.dtype(dtype).name}')
        r.r4(inp.pairs, None, dtype)
        assert_same({'R3': a, 'R4 with the diagonal in row N': r.step()}, 'R3')
        r.r4(inp.pairs, inp.snr, dtype)
        live = r.step()
        r.check(live, held, _rounded(inp.snr, dtype), tag=f'R4 {np.dtype(dtype).name}')
        for plane in ('BUF_SINR_DB', 'BUF_RATE_BPS', 'BUF_CAPACITY', 'BUF_REWARD'):        # the SNR row moves snr_db and nothing else
            assert np.array_equal(live[plane], a[plane]), plane
        assert not np.array_equal(live['BUF_SNR_DB'], a['BUF_SNR_DB'])
    shared = tr.pairs(c, True)
    r.r3(shared, np.float64)
    a = r.step()
    r.check(a, shared, tag='R3 shared')
    r.r3(_repeated(shared, c.b), np.float64)
    assert_same({'shared': a, 'repeated per env': r.step()}, 'shared')


@pytest.mark.parametrize('name', LARGE_HOST)
def test_host_link_table_in_three_chunks(rig, name):
    """R2 at 2 x 1100 x 1100 = 2.42 M entries: two staging blocks of 1 Mi entries, the third chunk reuses the first behind its event."""
    r = rig(name)
    inp = tr.inputs(name)
    assert inp.pairs.size > 2 << 20
    r.r2(inp.pairs)
    r.check(r.step(), inp.pairs, tag='R2')


@pytest.mark.parametrize('name', LARGE_DEVICE)
def test_device_routes_past_the_conversion_grid(rig, native, name):
    """R3 with more entries than one trip of gain_from_db_kernel's grid converts (num_cus x 32 x 256), R4 in float32."""
    r = rig(name)
    c = r.case
    inp = tr.inputs(name)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if 'R3f64' in c.routes:
        assert inp.pairs.size > cus * 32 * 256
        r.r3(inp.pairs, np.float64)
        r.check(r.step(), inp.pairs, tag='R3 float64')
    if 'R3f32shared' in c.routes:
        shared = tr.pairs(c, True)
        assert shared.size > cus * 32 * 256
        r.r3(shared, np.float32)
        r.check(r.step(), _rounded(shared, np.float32), tag='R3 float32 shared')
    r.r4(inp.pairs, inp.snr, np.float32)
    r.check(r.step(), _rounded(inp.pairs, np.float32), _rounded(inp.snr, np.float32), tag='R4 float32')


def test_more_links_than_the_library_takes_are_refused(native):
    """The 2100-link strided case of the case table is planned only: d2d_create takes at most D2D_MAX_LINKS = 2048 links."""
    from gym_d2d_amd.simulator import Simulator
    c = tr.BY_NAME['n2100_strided']
    assert c.n > native.MAX_LINKS
    with pytest.raises(native.NativeError) as exc:
        Simulator(dict(num_rbs=c.rbs, num_cues=c.cues, num_due_pairs=c.dues, num_envs=c.b), max_links=c.n)
    assert exc.value.code == native.ERR_INVALID


@pytest.mark.parametrize('name', tr.FLAG_CASES)
def test_live_table_domain_flags(rig, native, name):
    """PL_TABLE_DB: NaN and -inf raise FLAG_PATH_LOSS_DOMAIN only where the step reads them - in an interferer entry (j, i) of two links on
    one RB, in the env that holds it and in no other; not at a pair on different RBs; in row N of a link, which every step reads."""
    r = rig(name)
    c = r.case
    inp = tr.inputs(c.name)
    env = 3
    assert env not in tr.special_envs(c) and c.b > env
    rb = r.act.rb[env]
    alive = np.setdiff1d(np.arange(c.n), tr.dead_links(c))
    j, i = next((int(j), int(i)) for j in alive[::-1] for i in alive if i != j and rb[i] == rb[j])     # two links on one RB
    k = int(next(k for k in alive if rb[k] != rb[j]))
    r.r4(inp.pairs, inp.snr, np.float64)
    clean = r.step()
    assert not (clean['BUF_ENV_FLAGS'] & native.FLAG_PATH_LOSS_DOMAIN).any()
    n = c.n
    for value in (np.nan, -np.inf):
        for row, col, raised in ((j, i, True), (j, k, False), (n, i, True)):
            kept = r.live[env, row, col].item()
            r.live[env, row, col] = value
            flags = r.step()['BUF_ENV_FLAGS']
            r.live[env, row, col] = kept
            torch.cuda.synchronize()
            if raised:
                others = np.delete(np.arange(c.b), env)
                assert flags[env] & native.FLAG_PATH_LOSS_DOMAIN, (value, row, col)
                assert np.array_equal(flags[others], clean['BUF_ENV_FLAGS'][others]), (value, row, col)
            else:
                assert np.array_equal(flags, clean['BUF_ENV_FLAGS']), (value, row, col)
    assert_same({'clean': clean, 'restored': r.step()}, 'clean')
