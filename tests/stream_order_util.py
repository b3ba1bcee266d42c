"""The harness of tests/test_gpu_stream_order.py: twin envs, a calibrated GPU sleep and one case behind it.

VecD2DEnv promises of every torch-path call that it is "enqueued on torch's current stream, nothing is synchronised".  A case
checks that promise on a side stream (non-blocking: the null stream orders nothing against it) while the GPU still sleeps:

    reference env   the null stream, torch.cuda.synchronize() after every call (Synced)
    subject env     inside `with torch.cuda.stream(side)`: two warm rounds, then a sleep of at least 100 ms and at least 20 times
                    the measured host time of a round, an event `gate` right behind it, and the round under test

A round rewrites every device argument by torch ops (Args.refresh: the same seeded draws on both sides), steps the env and calls
the API under test; every result is cloned right behind its call.  Behind the round the subject allocates blocks of the sizes of
the temporaries the wrappers drop on return (packed `allowed` words, uint8 env masks) and fills them with zeros - all forbidden,
all masked out: the caching allocator hands the freed blocks out at once, and on one stream the fill lands behind their reader.
`gate.query()` must still be False when the host is through: nothing waited for the GPU.  Then the clones are compared with the
reference's as bytes - every kernel here is deterministic, so there is no tolerance.

Stale state is valid state: every argument lives in a buffer that is allocated and filled before the first sleep and rewritten
in place behind it, and both envs have completed rounds before, so a kernel that ran early reads last round's values and shows
as a failed comparison, never as a fault.
"""
from __future__ import annotations

import math
import time
from types import SimpleNamespace

import numpy as np
import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import NeighborObsFunction, SignalPlanesObsFunction
from gym_d2d_amd.mobility import GaussMarkovMobility
from gym_d2d_amd.path_loss import ArrayPathLoss, SpatialChannelPathLoss
from gym_d2d_amd.queues import PacketTraffic

# the smallest shape at which a misordered launch still shows: more than one wave of envs, odd link and RB counts, one mask word
B, C, P, R = 64, 9, 11, 7
N = C + P
K = 3                                                # candidates of evaluate(), neighbours of neighbors()
SHAPE = {'num_rbs': R, 'num_cues': C, 'num_due_pairs': P}
MIN_SLEEP_MS, MIN_RATIO = 100.0, 20.0

# host-side subsets: uploaded by the warm round, a repeat comes from the wrappers' caches
ADJUSTABLE = np.arange(N) % 3 != 0
MOVABLE = np.arange(N) % 4 != 1
MOVABLE5 = np.isin(np.arange(N), C + np.arange(0, 10, 2))            # 5 DUE pairs <= R: the one-to-one calls
MOVABLE4 = np.isin(np.arange(N), C + np.arange(1, 9, 2))             # 4 DUE pairs: 16 subsets per RB


class Neighbors3(NeighborObsFunction):
    k = K


class ShadowedCostHata(ArrayPathLoss):
    """examples/per_step_path_loss.py's model: COST-231 Hata + log-normal shadowing drawn on every evaluation."""
    per_step = True

    def compute(self, view):
        xp, log_f = view.xp, math.log10(self.carrier_freq_GHz * 1000.0)
        h_tx = view.tx_column(lambda d: d.antenna_height_m)
        h_rx = view.rx_column(lambda d: d.antenna_height_m)
        a_hrx = (1.1 * log_f - 0.7) * h_rx - (1.56 * log_f - 0.8)
        pl = 46.3 + 33.9 * log_f - 13.82 * xp.log10(h_tx) - a_hrx + (44.9 - 6.55 * xp.log10(h_tx)) * xp.log10(view.distance() / 1000.0)
        return pl + 6.0 * view.normal(0), xp.diagonal(pl, dim1=1, dim2=2) + 6.0 * view.normal(1)


class Urban(SpatialChannelPathLoss):
    """examples/spatial_channel.py's model."""
    median_kwargs = {'ple': 3.5}
    shadow_std_dB = 8.0
    decorrelation_m = 20.0
    fading = 'rayleigh'


STAGGER = np.arange(B) % 10
# feature set -> (config beyond SHAPE, VecD2DEnv keywords, reset keywords, whether the API arguments are made): the examples' own
# settings (mobility.py, packet_traffic.py, spatial_channel.py, per_step_path_loss.py, autoreset.py) at the shape above
FEATURES = {
    'plain': ({'obs_fn': SignalPlanesObsFunction}, {}, {}, True),
    'linear': ({}, {}, {}, False),
    'autoreset': ({}, {'autoreset': True}, {'elapsed': STAGGER}, False),
    'mobility': ({'obs_fn': SignalPlanesObsFunction}, {'mobility': GaussMarkovMobility(speed_std_mps=8.0, memory=0.8, dt_s=1.0)}, {}, False),
    'traffic': ({'obs_fn': SignalPlanesObsFunction},
                {'cue_actions': 'traffic', 'traffic': PacketTraffic(packets_per_step=1.5, packet_bits=1000, deadline_steps=4,
                                                                    buffer_bits=8 * 1000, dt_s=1e-3, p_on_to_off=0.2, p_off_to_on=0.2)},
                {}, False),
    'channel': ({'path_loss_model': Urban}, {'mobility': GaussMarkovMobility(speed_std_mps=2.0, memory=0.8)}, {}, False),
    'per_step': ({'path_loss_model': ShadowedCostHata, 'seed': 7}, {}, {}, False),
    'neighbor_obs': ({'obs_fn': Neighbors3}, {'autoreset': True}, {'elapsed': STAGGER}, False),
}


class Args:
    """Every device argument of one env, in buffers of its own: allocated and filled with valid values here, before any sleep,
    rewritten in place by refresh() with torch ops on the current stream."""

    def __init__(self, env, full: bool) -> None:
        dev = self.dev = env.device
        self.full = full
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        self.high = torch.as_tensor(np.asarray(env._initial_action_highs(), dtype=np.int32), device=dev)
        self.actions = z((B, env.num_agents), torch.int32)
        if not full:
            return
        levels = min(env.num_pwr_actions[k] for k in ('cue', 'due'))
        self.level_high = torch.full((N,), R * levels, dtype=torch.int32, device=dev)
        self.levels = levels
        f32, i32 = torch.float32, torch.int32
        self.allowed, self.env_mask = z((N, R), torch.bool), z((B,), torch.bool)
        self.adjustable, self.movable = z((N,), torch.bool), z((N,), torch.bool)
        self.target, self.floor = z((N,), f32), z((N,), f32)
        self.rb_cand, self.pw_cand, self.act_cand = z((B, K, N), i32), z((B, K, N), i32), z((B, K, N), i32)
        self.weights = z((B, 5, R), f32)
        self.link_pref, self.rb_pref = z((B, P, R), f32), z((B, P, R), f32)
        self.values = z((B, R, 16), torch.float64)
        self.quota = torch.ones((R,), dtype=i32, device=dev)
        self.power = z((B, N), i32)
        self.score, self.rx_thr = z((B, N, N), f32), z((B, N), f32)

    def refresh(self, gen) -> None:
        dev = self.dev
        rand = lambda shape: torch.rand(shape, generator=gen, device=dev)
        raw = torch.randint(0, 1 << 30, tuple(self.actions.shape), generator=gen, device=dev, dtype=torch.int32)
        torch.remainder(raw, self.high, out=self.actions)
        if not self.full:
            return
        torch.lt(rand((N, R)), 0.7, out=self.allowed)
        torch.lt(rand((B,)), 0.6, out=self.env_mask)
        torch.lt(rand((N,)), 0.7, out=self.adjustable)
        torch.lt(rand((N,)), 0.7, out=self.movable)
        torch.rand((N,), generator=gen, out=self.target).mul_(20.0).sub_(5.0)
        torch.rand((N,), generator=gen, out=self.floor).mul_(10.0).sub_(30.0)
        torch.randint(0, R, (B, K, N), generator=gen, out=self.rb_cand)
        torch.randint(0, self.levels, (B, K, N), generator=gen, out=self.pw_cand)
        raw = torch.randint(0, 1 << 30, (B, K, N), generator=gen, device=dev, dtype=torch.int32)
        torch.remainder(raw, self.level_high, out=self.act_cand)
        torch.rand((B, 5, R), generator=gen, out=self.weights).mul_(10.0)
        torch.rand((B, P, R), generator=gen, out=self.link_pref)
        torch.rand((B, P, R), generator=gen, out=self.rb_pref)
        torch.rand((B, R, 16), generator=gen, out=self.values)
        torch.randint(1, 3, (R,), generator=gen, out=self.quota)
        torch.randint(0, self.levels, (B, N), generator=gen, out=self.power)
        torch.rand((B, N, N), generator=gen, out=self.score).mul_(60.0).sub_(120.0)
        torch.rand((B, N), generator=gen, out=self.rx_thr).mul_(30.0).sub_(100.0)


class Synced:
    """The reference's face of an env: every call is followed by a device synchronise."""

    def __init__(self, env) -> None:
        self._env = env

    def __getattr__(self, name):
        attr = getattr(self._env, name)
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            res = attr(*args, **kwargs)
            torch.cuda.synchronize()
            return res
        return call


def make_side(feature: str, seed: int = 11):
    """One env of a feature set after reset(seed) on the null stream (reset() synchronises), with its arguments and generator."""
    config, kwargs, reset_kwargs, full = FEATURES[feature]
    env = VecD2DEnv({**SHAPE, **config}, num_envs=B, **kwargs)
    env.reset(seed=seed, **reset_kwargs)
    args = Args(env, full)
    gen = torch.Generator(device=env.device).manual_seed(seed)
    args.refresh(gen)
    torch.cuda.synchronize()
    return SimpleNamespace(env=env, args=args, gen=gen)


class Twins:
    """feature set -> (reference, subject), built on first use and again after a case that did not run to its end (its two envs
    may stand at different steps)."""

    def __init__(self) -> None:
        self.pairs, self.dirty = {}, set()

    def get(self, feature: str):
        if feature in self.dirty or feature not in self.pairs:
            self.drop(feature)
            self.pairs[feature] = (make_side(feature), make_side(feature))
        return self.pairs[feature]

    def drop(self, feature: str) -> None:
        for side in self.pairs.pop(feature, ()):
            side.env.close()
        self.dirty.discard(feature)

    def close(self) -> None:
        torch.cuda.synchronize()
        for feature in list(self.pairs):
            self.drop(feature)


def flatten(res):
    """The tensors of a result, in a fixed order: a tensor, a (named) tuple or list, a dict, None."""
    if res is None:
        return []
    if torch.is_tensor(res):
        return [res]
    if isinstance(res, dict):
        return [t for key in sorted(res) for t in flatten(res[key])]
    if isinstance(res, SimpleNamespace):
        return flatten(vars(res))
    if isinstance(res, (tuple, list)):
        return [t for part in res for t in flatten(part)]
    raise TypeError(f'no tensors in a {type(res).__name__}')


def one_round(env, args, gen, fn, steps: int, sync: bool = False) -> dict:
    """Fresh arguments, `steps` steps, then fn(env, args); every returned tensor cloned right behind its call."""
    out = {}
    for s in range(steps):
        args.refresh(gen)
        if sync:
            torch.cuda.synchronize()
        for k, t in enumerate(flatten(env.step(args.actions))):      # obs, rewards, dones and the info planes
            out[f'step{s}.{k}'] = t.clone()
    if fn is not None:
        for k, t in enumerate(flatten(fn(env, args))):
            out[f'result.{k}'] = t.clone()
    if sync:
        torch.cuda.synchronize()
    return out


def same_bytes(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def mismatches(got: dict, want: dict) -> list:
    """The names of the clones that differ from the reference's, byte for byte."""
    assert list(got) == list(want), (list(got), list(want))
    return [name for name in want if not same_bytes(got[name], want[name])]


class Harness:
    """The side stream and the calibrated sleep of one module."""

    def __init__(self, device) -> None:
        self.device = device
        self.side = torch.cuda.Stream(device=device)
        self.cycles_per_ms = self._calibrate()
        self.log = []                                # (case, sleep ms as slept, host ms of the warm round, of the round under test, gate still pending)

    def _calibrate(self, cycles: int = 20_000_000, trials: int = 5) -> float:
        """torch.cuda._sleep counts cycles of a clock this does not know: time a fixed count between two events a few times behind
        a warm-up and keep the median rate (now and then one sleep of a hundred runs nearly twice as fast as the others)."""
        torch.cuda._sleep(cycles)
        torch.cuda.synchronize()
        rates = []
        for _ in range(trials):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            torch.cuda.synchronize()
            rates.append(cycles / e0.elapsed_time(e1))
        return sorted(rates)[trials // 2]

    def sleep(self, ms: float, chunk_ms: float = 25.0) -> None:
        """Back-to-back sleeps of at most chunk_ms each: one that runs fast costs a fraction of the whole."""
        chunks = max(1, math.ceil(ms / chunk_ms))
        for _ in range(chunks):
            torch.cuda._sleep(int(ms / chunks * self.cycles_per_ms))

    def refill(self) -> list:
        """Blocks of the sizes the wrappers' temporaries had, zero-filled: no RB allowed, no env selected.  The packed words are
        4 N ceil(R / 32) bytes, pack_allowed's 64-bit steps 8 N and 256 N, an env mask B bytes."""
        words = 4 * N * ((R + 31) // 32)
        return [torch.zeros(nbytes, dtype=torch.uint8, device=self.device) for nbytes in (words, B, 8 * N, 256 * N) for _ in range(8)]

    def run(self, case: str, pair, fn=None, steps: int = 1) -> SimpleNamespace:
        """One case: the reference's three rounds, the subject's two warm rounds, the sleep, the round under test."""
        ref, sub = pair
        synced = Synced(ref.env)
        for _ in range(3):
            want = one_round(synced, ref.args, ref.gen, fn, steps, sync=True)
        side = self.side
        with torch.cuda.stream(side):
            one_round(sub.env, sub.args, sub.gen, fn, steps)          # binds the handle to the stream, allocates, fills the caches
            side.synchronize()
            t0 = time.perf_counter()
            keep = (one_round(sub.env, sub.args, sub.gen, fn, steps), self.refill())
            host_ms = (time.perf_counter() - t0) * 1e3
            side.synchronize()
            del keep
            sleep_ms = 1.25 * max(MIN_SLEEP_MS, MIN_RATIO * host_ms)  # a quarter above the floor: the clock may run faster than calibrated
            start, gate = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            self.sleep(sleep_ms)
            gate.record()
            t0 = time.perf_counter()
            got = one_round(sub.env, sub.args, sub.gen, fn, steps)
            spare = self.refill()
            pending = not gate.query()                                # the host is through and the GPU has not finished the sleep
            test_ms = (time.perf_counter() - t0) * 1e3
            side.synchronize()
            del spare
        slept_ms = start.elapsed_time(gate)
        self.log.append((case, slept_ms, host_ms, test_ms, pending))
        print(f'{case}: slept {slept_ms:.1f} ms, host time of the round {host_ms:.3f} ms warm / {test_ms:.3f} ms behind the sleep, '
              f'ratio {slept_ms / max(host_ms, test_ms):.0f}')
        return SimpleNamespace(got=got, want=want, pending=pending, slept_ms=slept_ms, host_ms=host_ms, test_ms=test_ms)
