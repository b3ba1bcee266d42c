"""The packet-traffic model of include/d2d_queue.h restated in NumPy integers and float64 - the yardstick of test_gpu_queue.py, checked
on its own by test_queue_cpu.py.  Built on the oracle's Philox4x32-10 (oracle/d2d_oracle.py) at the counter (global env index,
episode, step in the episode, link) and written from the header's formulas: nothing is imported from the package."""
import math

import numpy as np

from oracle import d2d_oracle as orc

SEED_MIX = 0x7061636B65747321
TABLE = 64
U32 = (1 << 32) - 1
INT_PLANES = ('arrived_bits', 'served_bits', 'expired_bits', 'overflow_bits', 'backlog_bits', 'hol_age_steps')
PLANES = INT_PLANES + ('mean_delay_steps', 'on')


def stream_seed(env_seed, seed=None):
    return int(seed) if seed is not None else (int(env_seed) ^ SEED_MIX) & (2 ** 64 - 1)


def threshold(p):
    """min(2^32 - 1, floor(p * 2^32))"""
    return min(U32, int(math.floor(p * 4294967296.0)))


def poisson_table(lam):
    """uint32 [64]: T_k = min(2^32 - 1, floor(c_k * 2^32)), c_k the running float64 sum of p_0 = exp(-lam), p_k = p_{k-1} lam / k."""
    out = np.empty(TABLE, dtype=np.uint32)
    p = math.exp(-lam)
    c = 0.0
    for k in range(TABLE):
        if k > 0:
            p = p * lam / k
        c = c + p
        out[k] = threshold(c)
    return out


def on_share(p_on_to_off, p_off_to_on):
    return 1.0 if p_on_to_off == 0 else p_off_to_on / (p_on_to_off + p_off_to_on)


def words(seed, first_env, episode, t, num_envs, num_links):
    """(w0, w1) uint32 [B, N]: the two draw words of step t of episode `episode`."""
    b = np.arange(num_envs, dtype=np.uint64)[:, None] + np.uint64(first_env)
    i = np.arange(num_links, dtype=np.uint64)[None, :]
    w = orc.philox4x32_10(b, np.uint64(episode), np.uint64(t), i, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return w[0], w[1]


def budget_bits(capacity_mbps, bits_per_mbps_step):
    """floor(double(capacity) * bits_per_mbps_step) clipped to [0, 2^31 - 1]; NaN, negative and zero give 0, +inf the clip."""
    with np.errstate(invalid='ignore', over='ignore'):
        x = np.asarray(capacity_mbps, dtype=np.float32).astype(np.float64) * np.float64(bits_per_mbps_step)
        pos = x > 0.0
        x = np.where(pos, np.minimum(x, 2147483647.0), 0.0)
        return np.floor(x).astype(np.int64)


class Restatement:
    """One batch of envs [B] with N = num_cues + num_due_pairs links each.  start(episode) is t = 0; step(capacity_mbps [B, N]) is
    the next step of the episode.  The planes are attributes (int64 but mean_delay_steps float32 and on uint8), ring is int64
    [D, B, N].  `events` counts, over every call, what the GPU test asserts each case exercises; `max_served_age` is the oldest age
    any served bit ever had."""

    def __init__(self, num_envs, num_cues, num_due_pairs, *, packets_per_step=(1.0, 1.0), packet_bits=12000, deadline_steps=8,
                 buffer_bits=None, dt_s=1e-3, p_on_to_off=0.0, p_off_to_on=1.0, seed=0, first_env=0):
        self.b, self.cues, self.n = num_envs, num_cues, num_cues + num_due_pairs
        rates = packets_per_step if isinstance(packets_per_step, (tuple, list)) else (packets_per_step, packets_per_step)
        self.rates = rates
        self.tables = np.stack([poisson_table(rates[0]), poisson_table(rates[1])])
        self.packet_bits, self.d = int(packet_bits), int(deadline_steps)
        self.buffer_bits = TABLE * self.packet_bits if buffer_bits is None else int(buffer_bits)
        assert 1 <= self.d <= 32 and self.packet_bits * TABLE < 2 ** 31 and 0 <= self.buffer_bits < 2 ** 31
        self.bits_per_mbps_step = 1e6 * dt_s
        self.thr_off, self.thr_on = threshold(p_on_to_off), threshold(p_off_to_on)
        self.thr_start = threshold(on_share(p_on_to_off, p_off_to_on))
        self.seed, self.first_env = int(seed), int(first_env)
        self.cls = (np.arange(self.n) >= num_cues).astype(np.int64)
        self.events = dict(expiry=0, overflow=0, partial=0, emptied=0, switched_on=0)
        self.max_served_age = 0
        self.episode = self.t = 0
        self.start(0)

    def start(self, episode):
        self.episode, self.t = int(episode), 0
        shape = (self.b, self.n)
        self.ring = np.zeros((self.d,) + shape, dtype=np.int64)
        for name in INT_PLANES:
            setattr(self, name, np.zeros(shape, dtype=np.int64))
        self.admitted_bits = np.zeros(shape, dtype=np.int64)
        self.mean_delay_steps = np.zeros(shape, dtype=np.float32)
        w0, _ = words(self.seed, self.first_env, self.episode, 0, self.b, self.n)
        self.on = ((w0 < np.uint32(self.thr_start)) | (self.thr_off == 0)).astype(np.uint8)
        return self

    def step(self, capacity_mbps):
        self.t += 1
        t, d, pkt = self.t, self.d, self.packet_bits
        w0, w1 = words(self.seed, self.first_env, self.episode, t, self.b, self.n)
        # 1  on/off source
        was_on = self.on.astype(bool)
        on = np.where(was_on, ~(w0 < np.uint32(self.thr_off)), w0 < np.uint32(self.thr_on))
        if self.thr_off == 0:
            on[:] = True
        self.events['switched_on'] += int((on & ~was_on).sum())
        # 2  arrivals
        k = (self.tables[self.cls][None, :, :] <= w1[:, :, None]).sum(axis=-1).astype(np.int64)
        k = np.where(on, k, 0)
        # 3  deadline
        s = t % d
        expired = self.ring[s].copy()
        self.ring[s] = 0
        kept = self.backlog_bits - expired
        assert (kept == self.ring.sum(axis=0)).all()
        # 4  finite buffer, tail drop
        n = np.minimum(k, (self.buffer_bits - kept) // pkt)
        assert (n >= 0).all()
        admitted = n * pkt
        self.ring[s] = admitted
        # 5  service, oldest first
        budget = budget_bits(capacity_mbps, self.bits_per_mbps_step)
        left = budget.copy()
        served = np.zeros_like(kept)
        weighted = np.zeros_like(kept)
        partial = np.zeros(kept.shape, dtype=bool)
        for age in range(d - 1, -1, -1):
            slot = (t - age) % d
            take = np.minimum(self.ring[slot], left)
            partial |= (take > 0) & (take % pkt != 0)
            if take.any():
                self.max_served_age = max(self.max_served_age, age)
            self.ring[slot] -= take
            left -= take
            served += take
            weighted += take * age
        backlog = self.ring.sum(axis=0)
        hol = np.zeros_like(kept)
        for age in range(d):                                  # the largest age with a non-empty cohort wins
            hol = np.where(self.ring[(t - age) % d] > 0, age, hol)
        with np.errstate(invalid='ignore', divide='ignore'):
            delay = np.where(served > 0, weighted.astype(np.float64) / served.astype(np.float64), 0.0).astype(np.float32)
        self.events['expiry'] += int((expired > 0).sum())
        self.events['overflow'] += int((k > n).sum())
        self.events['partial'] += int(partial.sum())
        self.events['emptied'] += int(((kept + admitted > 0) & (backlog == 0)).sum())
        self.on = on.astype(np.uint8)
        self.arrived_bits, self.admitted_bits, self.served_bits, self.expired_bits = k * pkt, admitted, served, expired
        self.overflow_bits, self.backlog_bits, self.hol_age_steps, self.mean_delay_steps = (k - n) * pkt, backlog, hol, delay
        return self

    def planes(self):
        """The planes in the kernel's dtypes."""
        out = {name: getattr(self, name).astype(np.int32) for name in INT_PLANES}
        out.update(mean_delay_steps=self.mean_delay_steps, on=self.on, ring=self.ring.astype(np.int32))
        return out
