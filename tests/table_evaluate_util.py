"""What the table what-if evaluation tests share (test_table_evaluate_cpu.py, test_gpu_table_evaluate.py): the case table of the
direct launches of csrc/d2d_evaltab.hip, seeded synthetic tables and candidate planes, the float64 reference on them, the LDS layout
restated, and the documented order of the total restated on the host.

The tables are drawn per (env, j, i) as table_route_util.pairs draws them (its _draw: own entries from the low range, every other
entry on its own from the wide one, link 1 dead where there is one): not symmetric, no two float64 entries equal, so a transposed or
mis-pitched index shows.  A float32 case holds the float32 rounding of its draw - 2^24 values cannot keep half a million draws apart,
so there the CPU test asserts what an index mistake needs instead: no entry equals its transpose or its neighbour in memory - and the
reference reads the rounded values.  The reference is evaluate_util.evaluate_ref on 'pl'."""
from functools import lru_cache

import numpy as np

import evaluate_util as evu
import table_route_util as tru
from oracle import d2d_oracle as orc

BAR = evu.BAR                                # the project's bar: |d| <= BAR max(|ref|, 1) on sinr_db (dB) and capacity_mbps (Mbps)
THRESHOLD_DB, THRESHOLD_CAP = evu.THRESHOLD_DB, evu.THRESHOLD_CAP
CHUNK, THREADS = 8, 256                      # include/d2d_evaltab.h: D2D_EVALTAB_CHUNK; csrc/d2d_evaltab.hip: ET_THREADS
P_LOW, P_HIGH = evu.P_LOW, evu.P_HIGH
DEAD_LINK = 1                                # its own entry is drawn from table_route_util.DEAD_DB: below the sensitivity, capacity 0

# links: (cues, due pairs)
SHAPES = {1: (1, 0), 3: (1, 2), 50: (20, 30), 130: (50, 80), 300: (100, 200)}
# (links, RBs, K, envs, entry type, rows per env beyond N): the path it forces.  K = 1, 8, 9, 17 are the chunk edges; B = 1 and 5;
# both entry widths; the table as [B, N, N] (0) and in the live layout [B, N+1, N] (1), whose last row is NaN: never read
CASES = (
    (1, 1, 9, 1, 'float64', 0),              # no interferer; a second workgroup with one candidate
    (3, 1, 8, 5, 'float32', 1),              # all links share the one RB; exactly one chunk
    (50, 6, 9, 5, 'float64', 1),             # one wave, not full
    (50, 6, 17, 1, 'float32', 0),            # three chunks, the last with one candidate
    (130, 70, 17, 5, 'float32', 1),          # three waves, the last with two lanes; mostly small groups
    (130, 70, 8, 1, 'float64', 0),
    (300, 2, 9, 1, 'float64', 1),            # groups of about 150 and more links than threads: the second pass of the loops
    (300, 2, 1, 5, 'float32', 0),            # one candidate
)


def lds_bytes(n, r):
    """The dynamic LDS a launch asks for, by the layout written in csrc/d2d_evaltab.hip: ca float4[N] | sens float[N] | txl
    float2[N] | key u32[N rounded up to 4] | srb int[N] | start int[R + 1] | wsum double[4] | wdom u32[4], each rounded up to 16."""
    r16 = lambda x: (x + 15) & ~15
    n4 = (n + 3) & ~3
    return 16 * n + r16(4 * n) + r16(8 * n) + 4 * n4 + r16(4 * n) + r16(4 * (r + 1)) + 32 + 16


def columns(n):
    """(ocols, link_tx, link_rx, d): the oracle's device columns and the default link list of a link count."""
    cues, dues = SHAPES[n]
    tx, rx, _ = tru.orc_links(cues, dues)
    return orc.device_columns(*orc.device_configs(cues, dues)[1:]), tx.astype(np.int32), rx.astype(np.int32), 1 + cues + 2 * dues


def draw_table(rng, b, n):
    """[B, N, N] float64 dB by (tx link j, rx link i), every entry drawn on its own (table_route_util._draw)."""
    eye = np.eye(n, dtype=bool)
    dead = np.zeros(n, dtype=bool)
    if n > DEAD_LINK:
        dead[DEAD_LINK] = True
    return tru._draw(rng, (b, n, n), eye[None], (eye & dead[None, :])[None])


def draw_planes(rng, b, k, n, r):
    """rb, pwr int32 [B, K, N]: rb uniform over the RBs with about a twelfth at -1 or R (on no RB); candidate 0 of env 0 has links
    0, 1, 2 on RB 0, the last link at -1 and the one before it at R, as far as there are that many links.  Powers as
    evaluate_util.make_case draws them."""
    rb = rng.integers(0, r, (b, k, n)).astype(np.int32)
    off = rng.random((b, k, n)) < 1 / 12
    rb[off] = rng.choice([-1, r], int(off.sum()))
    rb[0, 0, :3] = 0
    if n >= 4:
        rb[0, 0, -1] = -1
    if n >= 5:
        rb[0, 0, -2] = r
    if n == 1:
        rb[0, 0, 0], rb[0, 1 % k, 0] = -1, r
    elif n == 3:
        rb[0, 1 % k, -1], rb[0, 2 % k, 0] = -1, r
    pwr = rng.integers(P_LOW, P_HIGH + 1, (b, k, n)).astype(np.int32)
    end = rng.random((b, k, n))
    pwr[end < 1 / 3], pwr[end > 2 / 3] = P_LOW, P_HIGH
    return rb, pwr


@lru_cache(maxsize=None)
def make_case(n, r, k, b, dtype, extra):
    """The seeded case of a CASES entry: table (the array the kernel reads, [B, N + extra, N] of dtype, a NaN last row when extra),
    pl (what the reference reads: the entries as float64), the float64 draw, rb, pwr, the link list, the oracle's columns and the
    folded ones."""
    from gym_d2d_amd.sensing import fold_capacity_columns
    from gym_d2d_amd.table_evaluate import fold_table_columns
    rng = np.random.default_rng([n, r, k, b, len(dtype), extra])
    ocols, tx, rx, d = columns(n)
    draw = draw_table(rng, b, n)
    rb, pwr = draw_planes(rng, b, k, n, r)
    table = np.full((b, n + extra, n), np.nan, dtype=dtype)
    table[:, :n] = draw
    budget = {'eirp_off_db': ocols.eirp_off_db, 'rx_off_db': ocols.rx_off_db, 'noise_dbm': ocols.noise_dbm}
    c = dict(n=n, r=r, k=k, b=b, d=d, dtype=dtype, rows=n + extra, tx=tx, rx=rx, ocols=ocols, draw=draw, table=table,
             pl=table[:, :n].astype(np.float64), rb=rb, pwr=pwr, cols=fold_table_columns(budget),
             cap_cols=fold_capacity_columns({'bw_hz': ocols.bw_hz, 'sens_dbm': ocols.sens_dbm}))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def reference(c, rb=None, pwr=None, pl=None):
    """evaluate_ref on the case's table (or pl) for its planes (or rb / pwr): (sinr_db, capacity_mbps, total_mbps, decided) - decided
    False where the reference sinr_db lies within THRESHOLD_DB of the sensitivity."""
    rb, pwr = c['rb'] if rb is None else rb, c['pwr'] if pwr is None else pwr
    with np.errstate(all='ignore'):
        sinr, cap, total = evu.evaluate_ref(np.zeros((c['b'], c['d'], 2)), c['tx'], c['rx'], rb, pwr,
                                            {'ocols': c['ocols'], 'pl': c['pl'] if pl is None else pl}, c['r'])
    sens = c['ocols'].sens_dbm[np.asarray(c['rx'])]
    return sinr, cap, total, np.abs(sinr - sens[None, None, :]) > THRESHOLD_DB


@lru_cache(maxsize=None)
def case_ref(n, r, k, b, dtype, extra):
    """reference() of a CASES entry, computed once and left unchanged."""
    out = reference(make_case(n, r, k, b, dtype, extra))
    for v in out:
        v.setflags(write=False)
    return out


def total_in_order(cap, rb, r):
    """The total of one candidate as csrc/d2d_evaltab.hip forms it, on the host: cap float32 [N] and rb int [N] -> float32.  The
    links in sorted order (RB, link index; an rb outside [0, R) as the pseudo RB R); thread t adds the capacities of slots t,
    t + 256, ... in double; a butterfly over the 64 lanes of a wave (xor 32, 16, ... 1); the four wave sums in wave order; one
    rounding to float32."""
    cap, rb = np.asarray(cap, dtype=np.float32), np.asarray(rb, dtype=np.int64)
    n = len(cap)
    key = np.where((rb >= 0) & (rb < r), rb, r) * 2048 + np.arange(n)
    slots = np.zeros(-(-n // THREADS) * THREADS, dtype=np.float64)
    slots[:n] = cap[np.argsort(key, kind='stable')].astype(np.float64)
    part = np.zeros(THREADS, dtype=np.float64)
    for row in slots.reshape(-1, THREADS):
        part = part + row
    waves = part.reshape(THREADS // 64, 64)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lane ^ m]
    t = waves[0, 0]
    for w in range(1, THREADS // 64):
        t = t + waves[w, 0]
    return np.float32(t)


def totals_in_order(cap, rb, r):
    """total_in_order over [B, K, N] planes: float32 [B, K]."""
    b, k, _ = cap.shape
    return np.array([[total_in_order(cap[e, q], rb[e, q], r) for q in range(k)] for e in range(b)], dtype=np.float32)
