"""rollout_kernel (csrc/d2d_rollout.hip), the kernel the benchmark runs, in each of the 48 instantiations of launch_rollout - three
path-loss modes x (scalar records, nontemporal stores, padding, exact positions, one or two links per thread) - with every rare arm
driven on purpose: the 18 rows of tests/rollout_route_util.py under the path-loss models that make the library choose each mode
(PL_POWK twice: k = 4 and the general copy at k = 3), each by the Simulator shape and tuning keys test_rollout_route_cpu.py shows
the planner to answer with that kernel, and shows on the float64 reference to hold a link in every arm.  One test per (row, model):

    main     the eight envs: re-sorted sum, pool by selection, pool by sweep, out-of-range RBs and divided decode, pool order-free,
             the reward's second look, the row's edge links (shadowed link, both links of a thread, fixed links) in a pool, untouched
    roles    CueSinrShannon rows: twelve more steps, each member of env 5's twelve in turn the one non-D2D link below the threshold
    zero     a second batch: own link coincident alone and with company, an interferer on a receiver

Every output plane (SINR, SNR, rate, capacity, reward or reward_env, obs table and block, rb, pwr, env flags) is bound to a
guard_util.Guarded allocation and filled with a NaN pattern before each launch: afterwards the bands are intact, every word of a
plane the row's settings write is written, and a plane they switch off (no decoded actions, no obs table, the per-agent reward beside
reward_env) keeps the pattern.

Yardstick 1, bit equality on every plane: the rollout launch = the generic kernels' mask walk = their all-pairs sweep
(sim_util.search_variants), and three consecutive rollout launches (arrival order in the slots differs between launches).  The
zero-distance batch is held by this and by its flags alone: the oracle refuses such layouts.  Yardstick 2, oracle.d2d_oracle.step
with the row's PathLossSpec on the positions as uploaded (float64 under exact positions): |d| <= 1e-5 max(|ref|, 1) on sinr_db,
snr_db, rate_bps, capacity_mbps and the row's reward, no link left out (none lies within 1e-4 dB of a threshold: asserted on the
CPU); rb and pwr equal; the table rows equal to the position rows and the two planes' words; the LinearObs block equal to the
expansion of the table.  FLAG_RB_OUT_OF_RANGE exactly in env 3, FLAG_ZERO_DISTANCE exactly in the three coincident envs, no flag
anywhere else.

Measured on an MI355X (256 CUs): the worst deviation of any row, model, step and plane 2.8e-6 of the bar's max(|ref|, 1) (sinr_db,
o28_l1 at a log-distance exponent of 3.5; 1.5e-6 under the default model, 2.3e-6 with two links per thread), per row in
CHANGELOG.md; 72 tests in 6.4 s, none over 0.7 s (the first: library load), every other under 0.15 s.  Value-only mutations of the
kernel (rb_of under PL_POWK, the pool scans' RB test, the shadow's capacity, the pool in either second look) each fail here:
CHANGELOG.md."""
import json

import numpy as np
import pytest
import torch

import rollout_route_util as rr
from guard_util import Guarded
from oracle import d2d_oracle as orc
from sim_util import OUTS, assert_same

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC0BEEF                  # a quiet NaN as float32, an impossible rb / pwr / flag word as int32
FLOAT_PLANES = {'BUF_SINR_DB': 'sinr_db', 'BUF_SNR_DB': 'snr_db', 'BUF_RATE_BPS': 'rate_bps', 'BUF_CAPACITY': 'capacity_mbps'}


def _model_class(model):
    from gym_d2d_amd import path_loss as pl
    if model == 'hata':
        return pl.CostHataPathLoss
    ple = rr.spec(model).ple

    class Ple(pl.LogDistancePathLoss):
        def __init__(self, f):
            super().__init__(f, ple=ple)
    return Ple


class Rig:
    """A Simulator in the row's shape and settings, its output planes bound to guarded allocations."""

    def __init__(self, native, inp, tmp_path):
        from gym_d2d_amd.simulator import BASE_STATION_ID, Simulator
        self.native, self.inp, self.row = native, inp, inp.row
        row = inp.row
        cfg = dict(num_rbs=row.rbs, num_cues=row.cues, num_due_pairs=row.dues, num_envs=rr.B, path_loss_model=_model_class(inp.model))
        overrides = rr.device_overrides(row, inp.model)
        if overrides:
            cfg['device_config_file'] = tmp_path / 'devices.json'
            cfg['device_config_file'].write_text(json.dumps(overrides))
        self.sim = sim = Simulator(cfg, max_links=row.n)
        self.h = h = sim.handle
        sim.set_positions(inp.pos)
        keys = sim.default_link_keys()
        if inp.model == 'hata':                                   # the CUE links as downlinks
            keys = [(BASE_STATION_ID, cue) for cue in sim.devices.cues.keys()] + list(sim.devices.dues.keys())
        sim.set_links(keys)
        assert np.array_equal(sim.link_tx, inp.tx) and np.array_equal(sim.link_rx, inp.rx) and np.array_equal(sim.link_type, inp.ty)
        p = sim.config.num_pwr_actions
        assert np.array_equal(inp.levels, np.where(inp.ty == orc.SIDELINK, p['due'], np.where(inp.ty == orc.UPLINK, p['cue'], p['mbs'])))
        h.set_obs_mode({'none': native.OBS_NONE, 'table': native.OBS_TABLE, 'linear': native.OBS_LINEAR}[row.obs])
        h.set_reward(row.reward, inp.param)
        h.set_reward_layout(native.REWARD_PER_ENV if row.per_env else native.REWARD_PER_AGENT)
        h.set_export_actions(row.export)
        for key, value in row.tune:
            h.set_tuning(getattr(native, rr.TUNE_KEYS[key]), value)
        if inp.fixed is not None:
            h.set_fixed_actions(*inp.fixed)
        names = OUTS + (('BUF_REWARD_ENV',) if row.per_env else ()) + (('BUF_OBS',) if row.obs == 'linear' else ())
        self.planes = {}
        for name in names:
            which = getattr(native, name)
            g = Guarded(h.buffer_shape(which), torch.int32 if native.BUFFER_DTYPES.get(which, np.float32) == np.int32 else torch.float32)
            h.bind_buffer(which, g.array.data_ptr(), g.nbytes)
            self.planes[name] = g
        self.unwritten = set()
        if row.per_env:
            self.unwritten.add('BUF_REWARD')
        if row.obs == 'none':
            self.unwritten.add('BUF_OBS_TABLE')
        if not row.export:
            self.unwritten |= {'BUF_RB', 'BUF_PWR'}

    def close(self):
        self.h.synchronize()
        self.h.close()

    def launch(self, raw):
        for g in self.planes.values():
            g.array.view(torch.int32).fill_(PATTERN)
        torch.cuda.synchronize()
        self.sim.step_arrays(rr.handle_actions(self.inp, raw))
        self.h.synchronize()
        snap = {}
        for name, g in self.planes.items():
            assert g.intact(), (self.row.name, name)
            snap[name] = g.array.view(torch.int32).cpu().numpy().copy()
            if name in self.unwritten:
                assert (snap[name] == PATTERN).all(), (self.row.name, name, 'written although switched off')
            else:
                assert (snap[name] != PATTERN).all(), (self.row.name, name, int((snap[name] == PATTERN).sum()))
        return snap

    def variant(self, name):
        """sim_util.search_variants' settings; the generic kernels with the links per thread on auto (two per thread they sum the
        capacities over another wave partition, test_two_links_per_thread_matches_one), the rollout kernel with the row's."""
        bucket, walk = {'mask_walk': (True, 0), 'member_lists': (True, 2), 'all_pairs': (False, 0), 'auto': (True, -1)}[name]
        self.h.set_bucketing(bucket)
        self.h.set_tuning(self.native.TUNE_STEP_WALK, walk)
        self.h.set_tuning(self.native.TUNE_STEP_LPT, dict(self.row.tune).get('lpt', -1) if walk != 0 else -1)

    def variants(self, raw, canonical_nans=False):
        """One launch per search variant (member_lists and auto are both the rollout kernel) and a third rollout launch."""
        snaps = {}
        for name in ('mask_walk', 'member_lists', 'all_pairs', 'auto', 'third'):
            self.variant('auto' if name == 'third' else name)
            snaps[name] = self.launch(raw)
            if canonical_nans:
                for plane, words in snaps[name].items():
                    if plane not in ('BUF_RB', 'BUF_PWR', 'BUF_ENV_FLAGS'):
                        words[np.isnan(words.view(np.float32))] = 0x7FC00000
        return snaps

    def check(self, snap, ref, pos, tag):
        """Yardstick 2 on one snapshot; returns the worst deviation per plane."""
        row, inp = self.row, self.inp
        errs = {field: rr.rel_err(snap[name].view(np.float32), ref[field]) for name, field in FLOAT_PLANES.items()}
        if row.per_env:
            errs['reward'] = rr.rel_err(snap['BUF_REWARD_ENV'].view(np.float32), ref['reward'])
        elif row.reward == 1:
            reward = snap['BUF_REWARD']
            assert (reward == reward[:, :1]).all(), 'one scalar per env for every agent'
            errs['reward'] = rr.rel_err(reward[:, 0].view(np.float32), ref['reward'])
        else:
            errs['reward'] = rr.rel_err(snap['BUF_REWARD'].view(np.float32), ref['reward'])
        print(f'{row.name} {inp.model} {tag}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= rr.TOL, (row.name, inp.model, tag, k, v)
        if row.export:
            assert np.array_equal(snap['BUF_RB'], ref['rb']) and np.array_equal(snap['BUF_PWR'], ref['pwr'])
        if row.obs != 'none':
            self.check_table(snap, pos)
        return errs

    def check_table(self, snap, pos):
        """The obs table: the link's position row (float64 positions: their float32 roundings), then the SINR and SNR planes' words;
        the LinearObs block: the expansion of that table, word for word."""
        p32 = np.asarray(pos).astype(np.float32)
        table = snap['BUF_OBS_TABLE']
        assert np.array_equal(table[:, :, :2].view(np.float32), p32[:, self.inp.tx], equal_nan=True)
        assert np.array_equal(table[:, :, 2:4].view(np.float32), p32[:, self.inp.rx], equal_nan=True)
        assert np.array_equal(table[:, :, 4], snap['BUF_SINR_DB']) and np.array_equal(table[:, :, 5], snap['BUF_SNR_DB'])
        if self.row.obs == 'linear':
            assert np.array_equal(snap['BUF_OBS'], orc.expand_obs(table))


def _same(inp, snaps, ref_name='mask_walk'):
    """assert_same; a difference is reported by plane, env, link and the arm the reference puts the link in."""
    try:
        assert_same(snaps, ref_name)
    except AssertionError:
        arm, clear, _ = rr.classify(inp)
        lines = []
        for name, snap in snaps.items():
            for buf, ref in snaps[ref_name].items():
                where = np.argwhere(snap[buf] != ref)
                for w in where[:6]:
                    w = tuple(int(x) for x in w)
                    lines.append(f'{name} {buf} {w} {hex(snap[buf][w])} != {hex(ref[w])}' +
                                 (f' arm {arm[w[:2]]} clear {clear[w[:2]]}' if len(w) >= 2 and ref.shape[1] == inp.row.n else ''))
                if len(where):
                    lines.append(f'{name} {buf}: {len(where)} words differ')
        raise AssertionError('\n'.join(lines))


@pytest.fixture
def rig(native, tmp_path):
    rigs = []

    def make(name, model):
        rigs.append(Rig(native, rr.inputs(name, model), tmp_path))
        return rigs[-1]
    yield make
    for r in rigs:
        r.close()


@pytest.mark.parametrize('name,model', rr.CASES)
def test_rollout_route(rig, native, name, model):
    r = rig(name, model)
    inp, row, h = r.inp, r.row, r.h
    # ---- main: the generic kernels' mask walk and all-pairs sweep, and three rollout launches, bit for bit
    snaps = r.variants(inp.raw)
    _same(inp, snaps)
    got = snaps['auto']
    worst = r.check(got, inp.ref, inp.pos, 'main')
    want = np.zeros(rr.B, dtype=np.int32)
    want[3] = native.FLAG_RB_OUT_OF_RANGE
    assert np.array_equal(got['BUF_ENV_FLAGS'], want), got['BUF_ENV_FLAGS']
    assert h.status_flags() == native.FLAG_RB_OUT_OF_RANGE
    # ---- roles: each of env 5's twelve in turn the one non-D2D link below the threshold
    for k, s in enumerate(inp.roles):
        h.set_reward(row.reward, s.param)
        r.variant('auto')
        a = r.launch(s.raw)
        r.variant('mask_walk')
        _same(inp, {'rollout': a, 'mask_walk': r.launch(s.raw)}, 'rollout')
        errs = r.check(a, s.ref, inp.pos, f'role {k}')
        worst = {key: max(v, errs[key]) for key, v in worst.items()}
        assert np.array_equal(a['BUF_ENV_FLAGS'], want)
    print(f'WORST {name} {model} ' + json.dumps(worst))
    # ---- zero: coincident devices, by the bits and the flags alone
    h.set_reward(row.reward, inp.param)
    r.sim.set_positions(inp.zero_pos)
    # (a NaN is held as a NaN, as in test_rollout_kernel_zero_distance_own_link_matches_the_generic_kernels: under PL_POWK the sign
    # bit of the coincident link's NaN with company differs between launches of the same kernel)
    snaps = r.variants(inp.zero_raw, canonical_nans=True)
    _same(inp, snaps)
    got = snaps['auto']
    flags = got['BUF_ENV_FLAGS']
    assert (flags[:3] & native.FLAG_ZERO_DISTANCE).all() and (flags[3:] == 0).all(), flags
    assert not (flags & native.FLAG_RB_OUT_OF_RANGE).any()
    sinr = got['BUF_SINR_DB'].view(np.float32)
    for env, p in rr.ZERO_LINKS:
        assert not np.isfinite(sinr[env, row.cues + p]), (env, p, sinr[env, row.cues + p])
    assert np.isfinite(sinr[3:]).all()
    if row.obs != 'none':
        r.check_table(got, inp.zero_pos)
    if row.export:
        rb, pwr = orc.decode_actions(inp.zero_raw, inp.levels[None, :])
        assert np.array_equal(got['BUF_RB'], rb) and np.array_equal(got['BUF_PWR'], pwr)
