"""What the direct-launch queue tests share (test_element_direct_cpu.py, test_gpu_queue_direct.py): the seeded cases of
queue_step_kernel (csrc/d2d_queue.hip) past the small, benign parameters test_gpu_queue.py launches it at, each with the path it
forces, and their integer restatement (queue_util.Restatement), computed once per process and left unchanged.  Nothing is imported
from the package.

A case is a PROGRAM: the list of its launches, each with the clock it is launched at, the capacity plane it reads and the eight planes
and the ring as the restatement leaves them (the kernel's dtypes).  A lockstep case starts its episode at t = 0 and then visits the
steps `ts`; a jump from t = 0 to a far t with empty rings is a valid state (on the reference side: ref.t = t0 - 1).  The clock case
follows mobility_direct_util.clock_schedule with one single-env restatement per env."""
from functools import lru_cache

import numpy as np

import queue_util as qu
from mobility_direct_util import CLOCK_B, CLOCK_FIRST_ENV, clock_schedule

SEED = 77
PKT, DT = 1000, 1e-3
MAX_THREADS = 17219
BASE = dict(packets_per_step=(2.0, 0.7), packet_bits=PKT, buffer_bits=5 * PKT + 7, dt_s=DT, p_on_to_off=0.2, p_off_to_on=0.3)
BIG_PKT = 2 ** 25 - 1
EVENTS = ('expiry', 'overflow', 'partial', 'emptied', 'switched_on')

# name: B, CUEs, DUE pairs, D | the path it forces.  Unstated: the model BASE, steps 1 - 40, first_env 4096, episode 2, capacity 'synthetic'
CASES = {
    'one_link': dict(b=300, cues=1, pairs=0, d=8, capacity='by_env',
                     why='links = 1: the 0xFFFFFFFF reciprocal, every thread beyond 0 corrected; the CUE table only'),
    'due_only': dict(b=33, cues=0, pairs=64, d=3, why='n_cues == 0: i < cues never true; a power-of-two link count'),
    'wg_links': dict(b=9, cues=128, pairs=128, d=8, why='links = 256 = the workgroup: an env per workgroup exactly'),
    'odd': dict(b=67, cues=3, pairs=254, d=8, why='links 257, 17 219 threads: the last workgroup partly idle, envs straddle workgroups'),
    'limits': dict(b=5, cues=70, pairs=61, d=32, steps=80, capacity='limits',
                   model=dict(packets_per_step=(40.0, 12.0), packet_bits=BIG_PKT, buffer_bits=2 ** 31 - 1),
                   why='64-bit delay_sum, a backlog beside 2^31 - 1, the budget that saturates, k = 64'),
    'wrap31': dict(b=5, cues=70, pairs=61, d=3, ts=tuple(range(2 ** 31 - 5, 2 ** 31 + 7)), episode=2 ** 32 - 1, first_env=2 ** 32 - 5,
                   why='t mod D unsigned across t = 2^31; the episode and env counter words at 2^32 - 1'),
    'wrap32': dict(b=5, cues=70, pairs=61, d=7, ts=tuple(range(2 ** 32 - 12, 2 ** 32)), episode=2 ** 32 - 1, first_env=2 ** 32 - 5,
                   why='the last step counter, 2^32 - 1, with a D that does not divide 2^32'),
    'always_on': dict(b=5, cues=70, pairs=61, d=8, model=dict(p_on_to_off=0.0), why='p_on_to_off == 0: on forced at t = 0 and at every step'),
    'p_one': dict(b=5, cues=70, pairs=61, d=8, model=dict(p_on_to_off=1.0, p_off_to_on=1.0),
                  why='both switch thresholds clipped to 2^32 - 1: a link toggles at every step unless w0 is 2^32 - 1'),
    'no_buffer': dict(b=5, cues=70, pairs=61, d=8, model=dict(buffer_bits=PKT - 1),
                      why='buffer_bits < packet_bits: nothing is admitted, every arrival overflows'),
    'no_buffer_0': dict(b=5, cues=70, pairs=61, d=8, model=dict(buffer_bits=0), why='buffer_bits == 0: the same'),
    'clock': dict(b=CLOCK_B, cues=70, pairs=61, d=32, first_env=CLOCK_FIRST_ENV, why='the per-env clock: see clock_schedule'),
}
# the events a case cannot have (asserted to be 0); every other counter of every case is asserted to be above 0
NEVER = {'always_on': ('switched_on',), 'no_buffer': ('expiry', 'partial', 'emptied'), 'no_buffer_0': ('expiry', 'partial', 'emptied'),
         'clock': ('expiry',)}      # (no env of the clock case reaches step D = 32 in 31 launches)


def spec(name):
    s = dict(steps=40, first_env=4096, episode=2, capacity='synthetic')
    s.update(CASES[name])
    s['model'] = dict(BASE, **CASES[name].get('model', {}))
    s['n'] = s['cues'] + s['pairs']
    s.setdefault('ts', tuple(range(1, s['steps'] + 1)))
    return s


def restatement(name, num_envs=None, first_env=None):
    s = spec(name)
    return qu.Restatement(s['b'] if num_envs is None else num_envs, s['cues'], s['pairs'], deadline_steps=s['d'], seed=SEED,
                          first_env=s['first_env'] if first_env is None else first_env, **s['model'])


def launch_constants(name):
    """What the entry point takes beside the planes and the clock, from the restatement's own fields."""
    s, r = spec(name), restatement(name, 1)
    return dict(tables=r.tables, n_envs=s['b'], n_cues=s['cues'], n_due_pairs=s['pairs'], deadline_steps=s['d'],
                packet_bits=r.packet_bits, buffer_bits=r.buffer_bits, bits_per_mbps_step=r.bits_per_mbps_step,
                switches=(r.thr_off, r.thr_on, r.thr_start), first_env=s['first_env'], seed=SEED)


def synthetic_capacity(rng, b, n, by_env=False):
    """test_gpu_queue.py's plane, float32 [B, N] Mbps.  By link index mod 7 (by env index where an env has one link): 0, NaN, -1,
    1e-30 (no service: these queues fill, overflow and expire), +inf now and then (the queue empties), a whole number of packets
    (the budget lands on a packet boundary), anything (partial packets)."""
    cap = (rng.random((b, n)) * 3.0).astype(np.float32)
    col = np.broadcast_to(np.arange(b)[:, None] % 7 if by_env else np.arange(n)[None, :] % 7, (b, n))
    for c, v in enumerate((0.0, np.nan, -1.0, 1e-30)):
        cap[col == c] = np.float32(v)
    cap[(col == 4) & (rng.random((b, n)) < 0.3)] = np.inf
    whole = rng.integers(0, 4, (b, n)).astype(np.float32) * np.float32(PKT / (1e6 * DT))
    cap[col == 5] = whole[col == 5]
    return cap


# the budgets of the `limits` plane in bits, by link index mod 7; None: uniform up to 6 packets (column 4: +inf 3 steps in 10)
LIMIT_BUDGETS = (0, 2 ** 31 - 1, 2147483000, 2 ** 31 - 1, None, None, None)
LIMIT_MBPS = (0.0, 2147483.647, 2147483.0, 3e6)       # x 1000 bits per Mbps and step: 0; 2147483750 (float32), clipped; exact; 3e9, clipped


def limits_capacity(rng, b, n):
    cap = (rng.random((b, n)) * (6.0 * BIG_PKT / (1e6 * DT))).astype(np.float32)
    col = np.broadcast_to(np.arange(n)[None, :] % 7, (b, n))
    for c, v in enumerate(LIMIT_MBPS):
        cap[col == c] = np.float32(v)
    cap[(col == 4) & (rng.random((b, n)) < 0.3)] = np.inf
    return cap


def _capacity(s, rng, b):
    if s['capacity'] == 'limits':
        return limits_capacity(rng, b, s['n'])
    return synthetic_capacity(rng, b, s['n'], by_env=s['capacity'] == 'by_env')


def _planes(refs):
    """The planes of one restatement, or of one single-env restatement per env, in the kernel's dtypes."""
    if not isinstance(refs, list):
        return refs.planes()
    each = [r.planes() for r in refs]
    return {k: np.concatenate([p[k] for p in each], axis=1 if k == 'ring' else 0) for k in each[0]}


def _freeze(launch):
    for v in list(launch['want'].values()) + [launch['capacity']]:
        v.setflags(write=False)
    return launch


@lru_cache(maxsize=None)
def program(name):
    """(launches, stats).  A launch: dict(step, episode, capacity float32 [B, N], want: the nine arrays, clock: None or the launch
    of clock_schedule()).  stats: events (summed over the envs), max_served_age, k64 (draws of 64 arrivals), max_plane (the largest
    integer any plane or the ring ever held), max_backlog, max_product (the largest served_bits x mean_delay_steps of a link)."""
    s = spec(name)
    rng = np.random.default_rng([SEED, sorted(CASES).index(name)])
    b, n = s['b'], s['n']
    stats = dict(k64=0, max_plane=0, max_backlog=0, max_product=0.0)

    def look(refs):
        for r in refs if isinstance(refs, list) else [refs]:
            stats['k64'] += int((r.arrived_bits == 64 * r.packet_bits).sum())
            stats['max_plane'] = max([stats['max_plane'], int(r.ring.max())] + [int(getattr(r, p).max()) for p in qu.INT_PLANES])
            stats['max_backlog'] = max(stats['max_backlog'], int(r.backlog_bits.max()))
            stats['max_product'] = max(stats['max_product'], float((r.served_bits * r.mean_delay_steps.astype(np.float64)).max()))
    launches = []
    if name == 'clock':
        refs = [restatement(name, 1, CLOCK_FIRST_ENV + e) for e in range(b)]
        for k in clock_schedule():
            cap = _capacity(s, rng, b)
            for e, r in enumerate(refs):
                if k['flagged'][e]:
                    r.start(int(k['own_episode'][e]))
                else:
                    r.step(cap[e:e + 1])
                assert r.t == k['own_t'][e] and r.episode == k['own_episode'][e]
            look(refs)
            launches.append(_freeze(dict(step=None, episode=None, capacity=cap, want=_planes(refs), clock=k)))
    else:
        refs = restatement(name)
        refs.start(s['episode'])
        launches.append(_freeze(dict(step=0, episode=s['episode'], capacity=np.zeros((b, n), np.float32), want=_planes(refs), clock=None)))
        refs.t = s['ts'][0] - 1
        for t in s['ts']:
            cap = _capacity(s, rng, b)
            refs.step(cap)
            assert refs.t == t
            look(refs)
            launches.append(_freeze(dict(step=t, episode=s['episode'], capacity=cap, want=_planes(refs), clock=None)))
    every = refs if isinstance(refs, list) else [refs]
    stats['events'] = {k: sum(r.events[k] for r in every) for k in EVENTS}
    stats['max_served_age'] = max(r.max_served_age for r in every)
    return launches, stats
