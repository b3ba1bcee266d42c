"""The deviation kernels near their stated limits (test_deviation_large_cpu.py, test_gpu_deviation_large.py): three cases in
deviation_util's form, made by its generator (deviation_util.build_case), with their selections, their `allowed` masks and the
float64 oracle restricted to the groups an entry involves.  deviation_util.CASES stays as it is.

name          cues + dues   R     law    levels   selection                                   what it forces
d1950_r8      650 + 1300    8     ld2    16 + 16  40 links, 35 of them at 1024 or above,      W = 61 words per column, groups near 244, 163 168 B of LDS -
                                                  link N - 1 among them                       672 under the limit; two chunks of 32 links, the last with 8
d1100_r40     300 + 800     40    ld35   4 + 4    every 97th link (12)                        W = 35, an allowed mask of two words (N words = 2200), the
                                                                                              pow-k template past 64 KiB: 107 616 B with the mask
d300_r1024    100 + 200     1024  mixed  4 + 4    six links                                   R L = 4096: chunk == 1, grid.y == M; bits of 40 KiB; 32 allowed
                                                                                              words; 70 176 B without the mask, 108 576 B with it

evaluate() - the exact yardstick's source of planes - serves all three shapes as they stand (64 bytes per link under 'ld2', 80 under
a power law: 124 896, 88 208 and 28 144 bytes of its own LDS by evaluate_util.lds_bytes), so no case had to shrink.  'mixed' has no oracle model.

The restricted oracle.  An oracle launch costs K N^2, and groups do not interact: every quantity of link i's row (r, l) is a sum over
group(r) u {i}, D(c,p) one over group(c).  `restricted_planes` therefore runs the oracle once per RB r on the links of
group(c) u group(r) u {i} alone - the rows of r, the held row and the row with i gone - and leaves every other word of the [K, N]
planes NaN, so that a read outside the groups would show.  test_deviation_large_cpu.py shows deviation_util.by_oracle on these
planes equal to the full form on the existing d40_r2 and d50_r25 (`near` and `open` equal, `gain` to 1e-12 max(|ref|, 1): float64
on the same operands, the order of at most 50 terms apart).  `delta` and `total`, sums over ALL links, are NaN in this form."""
from functools import lru_cache

import numpy as np

import deviation_util as du
from oracle import d2d_oracle as orc

TIE = 1e-12                                          # restricted against full: |d| <= TIE max(|ref|, 1)
MAX_LDS_BYTES = 160 * 1024                           # D2D_DEVIATE_MAX_LDS_BYTES
LDS_64K = 64 * 1024                                  # csrc/d2d_addon.h launch(): past this the dynamic-LDS attribute is set first
MIN_GAIN = 0.5                                       # Mbps, test_gpu_deviation.py's

# deviation_util.CASES' form; `oracle` = (envs, the selected links the float64 side takes)
CASES = {
    'd1950_r8': dict(cues=650, dues=1300, r=8, law='ld2', cell=500.0, b=2, no_rb=0, cue_max=15, due_max=15, oracle=(1, (5, 650, 1024, 1949))),
    'd1100_r40': dict(cues=300, dues=800, r=40, law='ld35', cell=500.0, b=2, no_rb=0, cue_max=3, due_max=3, oracle=(1, (0, 291, 679, 1067))),
    'd300_r1024': dict(cues=100, dues=200, r=1024, law='mixed', cell=500.0, b=2, no_rb=0, cue_max=3, due_max=3, oracle=None),
}
# name: (LDS bytes without an allowed mask, with one)
LDS = {'d1950_r8': (163168, 170976), 'd1100_r40': (98816, 107616), 'd300_r1024': (70176, 108576)}
MASKED = ('d1100_r40', 'd300_r1024')                 # d1950_r8 takes no mask: with one it no longer fits - the first refusal
ORACLE_CASES = tuple(name for name, k in CASES.items() if k['oracle'] is not None)
ONLY_1023 = 1                                        # d300_r1024: the selected link (by position) whose mask allows RB 1023 alone


@lru_cache(maxsize=None)
def make_case(name):
    """deviation_util.build_case of a CASES entry, computed once."""
    return du.build_case(name, CASES[name])


def selection(name):
    """The selected links of a case: ascending, distinct, non-contiguous."""
    n = CASES[name]['cues'] + CASES[name]['dues']
    if name == 'd1950_r8':
        return np.unique(np.concatenate([[5, 333, 649, 650, 1023], np.arange(1024, n - 1, 28), [n - 1]]))
    if name == 'd1100_r40':
        return np.arange(0, n, 97)
    return np.array([0, 57, 99, 100, 211, n - 1])


def chunking(name):
    """(chunk, workgroups per env) by prepare() of csrc/d2d_deviate.hip: a chunk takes links until it has about 4096 entries."""
    k = CASES[name]
    m = len(selection(name))
    entries = k['r'] * (max(k['cue_max'], k['due_max']) + 1)
    chunk = min(256, m, max(1, -(-4096 // entries)))
    return chunk, -(-m // chunk)


def oracle_links(name):
    """(envs, links) the float64 side takes of a case; None where the law has no oracle model."""
    if CASES[name]['oracle'] is None:
        return None
    envs, links = CASES[name]['oracle']
    return np.arange(envs), np.asarray(links)


def allowed_mask(name):
    """The bool [N, R] mask of a MASKED case.  d1100_r40: deviation_util.allowed_mask - random at 60 %, a fifth of the rows empty,
    every third link's own RB excluded.  d300_r1024: only the last word, RBs 992 .. 1023, and for one selected link RB 1023 alone."""
    c = make_case(name)
    if name == 'd1100_r40':
        return du.allowed_mask(c.n, c.r, 5, c.rb[0])
    assert name == 'd300_r1024'
    mask = np.zeros((c.n, c.r), dtype=bool)
    mask[:, 992:] = True
    mask[selection(name)[ONLY_1023]] = False
    mask[selection(name)[ONLY_1023], c.r - 1] = True
    return mask


# ------------------------------------------------------------------------------------------ the oracle on the groups involved
_kept = {}


def restricted_planes(c, e, i, rb_rows, pwr_rows):
    """deviation_util.oracle_planes for the variants of link i (deviation_util.variants: K = R Lmax + 1 rows that differ from the
    held state in link i alone), computed per RB r on group(c) u group(r) u {i}: float64 (sinr_db, capacity_mbps) [K, N], NaN
    outside.  The held row is the first row that has link i at its own (rb, power); kept per (case, env, link)."""
    key = (c.name, int(e), int(i))
    if key in _kept:
        return _kept[key]
    rb_rows, pwr_rows = np.asarray(rb_rows, dtype=np.int64), np.asarray(pwr_rows, dtype=np.int64)
    k, n = rb_rows.shape
    lmax = (k - 1) // c.r
    held_rb, held_pw = rb_rows[k - 1].copy(), pwr_rows[k - 1].copy()
    cur = int(np.asarray(c.rb)[e][i])
    held_rb[i] = cur
    assert np.array_equal(held_rb, np.asarray(c.rb)[e]) and np.array_equal(held_pw, np.asarray(c.pwr)[e]), 'variants of the case state'
    sinr, cap = np.full((k, n), np.nan), np.full((k, n), np.nan)
    on_cur = (held_rb == cur) & (0 <= cur < c.r)
    held = np.flatnonzero((rb_rows[:k - 1, i] == cur) & (pwr_rows[:k - 1, i] == held_pw[i]))
    for r in range(c.r):
        members = np.flatnonzero(on_cur | (held_rb == r) | (np.arange(n) == i))
        rows = np.concatenate([np.arange(r * lmax, (r + 1) * lmax), held[:1], [k - 1]])
        sub_rb = rb_rows[np.ix_(rows, members)]
        off = (sub_rb < 0) | (sub_rb >= c.r)
        sub_rb = np.where(off, c.r + np.arange(members.size)[None, :], sub_rb)        # a link on no RB shares its pseudo RB with nobody
        pos = np.broadcast_to(c.pos[e].astype(np.float64), (rows.size,) + c.pos[e].shape)
        out = orc.step(pos, np.asarray(c.tx)[members], np.asarray(c.rx)[members], sub_rb, pwr_rows[np.ix_(rows, members)].astype(np.float64),
                       c.cols, du.au._table_spec(c, e), chunk=rows.size)
        sinr[np.ix_(rows, members)], cap[np.ix_(rows, members)] = out['sinr_db'], out['capacity_mbps']
    _kept[key] = (sinr, cap)
    return _kept[key]


def by_oracle_restricted(c, envs, links, allowed=None, floor=None, min_gain=0.0):
    """deviation_util.by_oracle on restricted_planes."""
    return du.by_oracle(c, envs, links, allowed, floor, min_gain, planes=restricted_planes)


@lru_cache(maxsize=None)
def oracle_side(name, floors='none'):
    """by_oracle_restricted of a large case on its oracle envs and links under a floor setting, computed once."""
    envs, links = oracle_links(name)
    return by_oracle_restricted(make_case(name), envs, links, None, du.FLOOR_SETTINGS[floors])


# ------------------------------------------------------------------------------------------ the refusals
def largest_links(r, allowed=False):
    """The largest N that deviation_util.lds_bytes admits on r RBs (0: none)."""
    n = 0
    while n < 2048 and du.lds_bytes(n + 1, r, allowed) <= MAX_LDS_BYTES:
        n += 1
    return n
