"""The case tables and generators of the matching and colouring kernels near their stated limits - 2048 links, 160 KiB of LDS, wide
`allowed` masks, 64 power levels, a thread of the matching that owns up to 27 columns (test_solver_large_cpu.py,
test_gpu_assign_large.py, test_gpu_color_large.py).  The float64 references and restatements are the existing ones: assign_util's
weights_ref / solve_ref, assignpwr_util's weights_power_ref / best_power, color_util's color_graph.  Every reference is computed
once per process and left unchanged.  The tables of assign_util, assignpwr_util and color_util stay as they are: what
test_assign_cpu.py and its siblings assert about them does not move."""
from functools import lru_cache

import numpy as np

import assign_util as asu
import assignpwr_util as apu
import color_util as cu

MAX_LDS_BYTES = 160 * 1024                   # D2D_ASSIGN_MAX_LDS_BYTES, D2D_ASSIGNPWR_MAX_LDS_BYTES, D2D_COLOR_MAX_LDS_BYTES
SOLVE_THREADS = 256                          # a matching thread owns the columns tid + 256 q and marks them in bit q of `scanned`

# ------------------------------------------------------------------------------------------ 1. the weights kernel
# (cues, due pairs, RBs, law) -> (LDS bytes, the path it forces).  The movable links are the DUE links.
WEIGHT_CASES = {
    (1024, 1024, 64, 'ld35'): (155920, 'N = 2048: every movable j >= 1024 (the background is the CUE links, j < 1024), walks of 5 to 24 members, M > R'),
    (48, 2000, 256, 'mixed'): (156688, '2000 movable links, 500 per wave; mostly empty RBs'),
    (1500, 548, 600, 'ld2'): (141680, 'the inverse-square law near the limit; ten lane trips over r'),
    (700, 330, 330, 'mixed'): (79648, 'M = R exactly'),
}
# once more with links = arange(1, N, 3) - CUE and DUE links alike - and `allowed` at about 70 %: (words, bits of the last word)
MASKED_CASES = {(1500, 548, 600, 'ld2'): (19, 24), (700, 330, 330, 'mixed'): (11, 10)}
# objective 'own' against evaluate(), bit for bit: -> the movable links.  evaluate() keeps 80 bytes per link under a power law, so
# it serves 2048 links under 'ld2' only; there the background has members on both sides of link 1024
OWN_CASES = {(1024, 1024, 64, 'ld2'): (1024, 1500, 2046, 2047), (700, 330, 330, 'mixed'): (3, 699, 700, 1029)}
OWN_LDS_BYTES = {(1024, 1024, 64, 'ld2'): 139536, (700, 330, 330, 'mixed'): 79648}
RELAUNCH_CASE = (1024, 1024, 64, 'ld35')     # a second launch and pointers moved by 4 bytes give the same bits


@lru_cache(maxsize=None)
def weights_case_ref(cues, dues, r, law):
    """asu.weights_ref of a WEIGHT_CASES entry, the DUE links movable."""
    c = asu.case(cues, dues, r, law)
    return asu.weights_ref(c, asu.due_links(c, cues))


def masked_movable(c):
    """(links int32 [M], allowed bool [N, R]) of a MASKED_CASES entry: every third link from link 1 on, about 70 % of the entries
    allowed (seeded); links[1] may take RB R - 1 alone - the last bit of the last word - and links[2] nothing at all."""
    rng = np.random.default_rng(5)
    links = np.arange(1, c['n'], 3, dtype=np.int32)
    allowed = rng.random((c['n'], c['r'])) < 0.7
    allowed[links[1]] = False
    allowed[links[1], c['r'] - 1] = True
    allowed[links[2]] = False
    return links, allowed


def with_tail_bits(words, r):
    """The packed words [N, ceil(R / 32)] with every bit at and above R of each last word set: a kernel must not read them."""
    out = np.array(words, dtype=np.uint32)
    if r & 31:
        out[:, -1] |= np.uint32((0xFFFFFFFF << (r & 31)) & 0xFFFFFFFF)
    return out


@lru_cache(maxsize=None)
def masked_case_ref(cues, dues, r, law):
    c = asu.case(cues, dues, r, law)
    return asu.weights_ref(c, masked_movable(c)[0])


@lru_cache(maxsize=None)
def own_case_ref(cues, dues, r, law):
    c = asu.case(cues, dues, r, law)
    return asu.weights_ref(c, np.asarray(OWN_CASES[(cues, dues, r, law)], dtype=np.int32))


# ------------------------------------------------------------------------------------------ 2. the matching
# on weight planes: (cues, dues, RBs, law), the DUE links movable, unmasked and masked at 60 % with allowed[j, j % R] kept
PLANE_CASES = ((1500, 548, 600, 'ld2'), (700, 330, 330, 'mixed'))


def plane_allowed(c):
    """bool [N, R]: about 60 % allowed, allowed[j, j % R] kept, so a complete matching stays."""
    rng = np.random.default_rng(5)
    allowed = rng.random((c['n'], c['r'])) < 0.6
    allowed[np.arange(c['n']), np.arange(c['n']) % c['r']] = True
    return allowed


def plane_conditions(w, col, feasible):
    """What a matching on a weight plane must have reached, asserted on the reference planes (CPU) and on the planes the kernel
    solved (GPU): every env feasible, a matched column a thread marks in bit 1 of `scanned` or above (>= 256), and at 600 RBs one in
    bit 2 (>= 512).  Returns (matched columns >= 256, >= 512)."""
    assert all(int(f) == 1 for f in feasible)
    col = np.asarray(col)
    high, higher = int((col >= SOLVE_THREADS).sum()), int((col >= 2 * SOLVE_THREADS).sum())
    assert high >= 1
    assert higher >= 1 or w.shape[-1] <= 2 * SOLVE_THREADS
    return high, higher


@lru_cache(maxsize=None)
def plane_ref(cues, dues, r, law, masked):
    """(w float32 [B, M, R], col int32 [B, M], value float32 [B], feasible [B]): the matching of the REFERENCE planes rounded to
    float32, by asu.solve_ref - what test_solver_large_cpu.py asserts feasibility and the column counts on."""
    own, harm, _ = weights_case_ref(cues, dues, r, law)
    w = (own - harm).astype(np.float32)
    if masked:
        c = asu.case(cues, dues, r, law)
        w = np.where(plane_allowed(c)[asu.due_links(c, cues)][None], w, -np.inf).astype(np.float32)
    res = [asu.solve_ref(w[e]) for e in range(w.shape[0])]
    return w, np.stack([x[0] for x in res]), np.asarray([x[1] for x in res], dtype=np.float32), np.asarray([x[2] for x in res])


def low_rank(m, r, seed):
    """float32 [m, r]: row effect + column effect + a little noise.  Every row wants the same columns, so rows displace one another
    along alternating paths - the opposite of asu.solve_matrix, whose independent normals are matched almost greedily."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 5, (m, 1)) + rng.normal(0, 5, (1, r)) + rng.normal(0, 0.01, (m, r))).astype(np.float32)


# name -> (rows, columns, the seeds of its envs, LDS bytes, the q = column // 256 of the highest matched column of env 0)
SYNTHETIC = {
    'integers 0 .. 3, 600 x 600': (600, 600, (8,), 21696, 2),
    'chain of 600': (600, 600, (0,), 21696, 2),
    'low rank 500 x 700': (500, 700, (9,), 22896, 2),
    'low rank 300 x 2600': (300, 2600, (11,), 66096, 10),
    'low rank 64 x 6000': (64, 6000, (11, 12), 144864, 23),
    'low rank 8 x 6800': (8, 6800, (11, 12), 163392, 21),
}
WIDE = 'low rank 300 x 2600'                 # the infeasible envs are made from this shape
WIDE_SEEDS = (11, 12, 13)
WIDE_ROWS = (7, 150)                         # the two rows of the middle env that may take the last column alone


def synthetic_matrix(name, seed):
    m, r = SYNTHETIC[name][:2]
    if name.startswith('integers'):
        return np.random.default_rng(seed).integers(0, 4, (m, r)).astype(np.float32)
    if name.startswith('chain'):
        return asu.chain_matrix(m)
    return low_rank(m, r, seed)


@lru_cache(maxsize=None)
def solved(name, seed):
    """(w, col, value, feasible) of one synthetic matrix by asu.solve_ref; the matrix is float32, so it is the one launched."""
    w = synthetic_matrix(name, seed)
    w.setflags(write=False)
    return (w,) + asu.solve_ref(w)


def row_greedy(w):
    """(col [M], value): every row in turn takes the best free column (equal values: the lowest); -1 and -inf where none is finite."""
    w = np.asarray(w, dtype=np.float64)
    free = np.ones(w.shape[1], bool)
    col, value = np.full(w.shape[0], -1), 0.0
    for a in range(w.shape[0]):
        j = int(np.argmax(np.where(free, w[a], -np.inf)))
        if not free[j] or not np.isfinite(w[a, j]):
            return col, -np.inf
        col[a], free[j] = j, False
        value += w[a, j]
    return col, value


def infeasible_batches():
    """[(name, w float32 [3, 300, 2600], the env that cannot be matched)]: in the middle env rows WIDE_ROWS may take column 2599
    only - the second of them reaches it through a thread's eleventh column and finds its owner with nowhere to go; and the same
    with a row of -inf."""
    base = np.stack([solved(WIDE, s)[0] for s in WIDE_SEEDS])
    two = base.copy()
    for a in WIDE_ROWS:
        two[1, a] = -np.inf
        two[1, a, -1] = 1.0 + a
    none = base.copy()
    none[1, WIDE_ROWS[1]] = -np.inf
    return [('two rows that may take column 2599 only', two, 1), ('a row of -inf', none, 1)]


# ------------------------------------------------------------------------------------------ 3. joint RB and power
# without floors, bit for bit against the per-level launches: (cues, dues, RBs, law) -> [(p_min, p_max) of every link]
EXACT_CASES = {
    (1024, 1024, 256, 'mixed'): ((0, 8),),                 # 156 688 bytes, all 1024 DUE links movable, nine launches
    (13, 50, 64, 'mixed'): ((-32, 31), (-31, 31)),         # 64 levels, D2D_ASSIGNPWR_MAX_LEVELS: eight full chunks; and 63
}
EXACT_SCATTERED = (700, 330, 330, 'mixed')                 # masked_movable(), apu.SCATTERED_BOUNDS by class, the 11-word allowed
# with floors: (cues, dues, RBs, law) -> (every STRIDE-th DUE link is movable, (p_min, p_max))
FLOOR_CASES = {
    (1024, 1024, 256, 'mixed'): (32, (0, 8)),              # M = 32, every movable j >= 1024
    (700, 330, 330, 'mixed'): (4, (0, 20)),                # M = 83
}


def floor_links(c, cues, dues, r, law):
    return asu.due_links(c, cues)[::FLOOR_CASES[(cues, dues, r, law)][0]]


UNREACHABLE_DB = 200.0


def unreachable_floors(c, cues, dues, r, law):
    """float64 [N]: the stricter apu.FLOOR_SETTINGS entry with the floor of every eighth movable link at UNREACHABLE_DB, which no
    power level gives: those links' rows have no admissible RB at all.  Under the two FLOOR_SETTINGS alone the reference leaves no
    row of either case without one (test_solver_large_cpu.py prints the shares), so the route of a whole row of -inf / NO_POWER at
    these shapes is taken by this third setting."""
    floor = apu.class_floors(c, cues, apu.FLOOR_SETTINGS[-1])
    floor[floor_links(c, cues, dues, r, law)[::8]] = UNREACHABLE_DB
    return floor


@lru_cache(maxsize=None)
def floor_case_ref(cues, dues, r, law):
    """apu.weights_power_ref of a FLOOR_CASES entry under no floors, every apu.FLOOR_SETTINGS entry and unreachable_floors():
    (w, valid, [(adm, near)] in the order (None, *FLOOR_SETTINGS, unreachable))."""
    c = asu.case(cues, dues, r, law)
    lo, hi = apu.uniform_bounds(c, *FLOOR_CASES[(cues, dues, r, law)][1])
    settings = [apu.class_floors(c, cues, pair) for pair in (None,) + apu.FLOOR_SETTINGS] + [unreachable_floors(c, cues, dues, r, law)]
    return apu.weights_power_ref(c, floor_links(c, cues, dues, r, law), lo, hi, floors=settings)


# ------------------------------------------------------------------------------------------ 4. the colouring
# cu.synthetic(b, n, r, **how) -> (how, LDS bytes, the path)
COLOR_CASES = {
    (1, 1025, 24): (dict(half=False, masked=False, bias=True, density=0.02), 152032, 'W = 33, a row word of one bit; five c0 trips'),
    (1, 1024, 33): (dict(half=True, masked=True, bias=False, density=0.02), 160112, 'W = 32 exactly; a 1-bit tail word of allowed'),
    (2, 300, 300): (dict(half=True, masked=True, bias=True, density=0.5), 42112, '10 words; the second trip of the r loops'),
    (2, 260, 257): (dict(half=False, masked=False, bias=True, density=0.9), 24032, 'proper on 257 RBs when spreading: RB 256 taken'),
    (1, 200, 1000): (dict(half=False, masked=True, bias=False, density=0.3), 67392, '32 words, an 8-bit tail; past 64 KiB by the RBs'),
    (1, 600, 70): (dict(half=False, masked=False, bias=False, density=0.5), 60656, 'mostly forced turns at three words'),
    (9, 130, 96): (dict(half=True, masked=True, bias=True, density=0.4), 8176, 'B = 9; R % 32 == 0 with a mask'),
}
# the complete graph on more than 256 RBs: (links, RBs) -> (LDS bytes, conflicts = sum of C(load, 2) with loads that differ by <= 1)
COMPLETE_CASES = {(300, 260): (28592, 40), (520, 257): (62512, 269)}


@lru_cache(maxsize=None)
def color_case(b, n, r):
    return cu.synthetic(b, n, r, **COLOR_CASES[(b, n, r)][0])


@lru_cache(maxsize=None)
def color_ref(b, n, r, pack):
    c = color_case(b, n, r)
    return cu.color_graph(c.score, c.tx_bias, c.rx_thr, c.rb, c.r, c.movable, c.allowed, pack)


def complete_inputs(m):
    """(score [1, m, m], rx_thr [1, m], rb [1, m]) of K_m: every score 1 against thresholds of 0, everybody on RB 0 before."""
    return np.ones((1, m, m), dtype=np.float32), np.zeros((1, m), dtype=np.float32), np.zeros((1, m), dtype=np.int32)


@lru_cache(maxsize=None)
def complete_ref(m, r, pack):
    score, thr, rb = complete_inputs(m)
    return cu.color_graph(score, None, thr, rb, r, None, None, pack)


def color_reaches(key, c, turn, refs):
    """The conditions a COLOR_CASES row claims, asserted on the outputs `refs` = {pack: (rb, conflicts, rbs_used, proper)} - the
    restatement's on the CPU, the kernel's on the GPU (they are equal there)."""
    b, n, r = key
    words = (r + 31) // 32
    chosen = {pack: out[0][:, turn] for pack, out in refs.items()}
    for pack, rbs in chosen.items():
        assert ((rbs >= 0) & (rbs < r)).all()
    if key == (1, 1025, 24):
        assert (n + 31) // 32 == 33 and n % 32 == 1 and -(-n // 256) == 5 and c.allowed is None
    if key == (1, 1024, 33):
        assert n % 32 == 0 and n // 32 == 32 and r % 32 == 1 and words == 2 and c.allowed is not None
        assert (chosen[False] == 32).any()                               # the one bit of the tail word is chosen
    if key == (2, 300, 300):
        assert words == 10 and all((rbs >= 256).any() for rbs in chosen.values())
    if key == (2, 260, 257):
        assert refs[False][3].tolist() == [1, 1] and refs[False][2].tolist() == [257, 257] and (chosen[False] == 256).any()
    if key == (1, 200, 1000):
        assert words == 32 and r % 32 == 8 and (chosen[False] >= 992).any() and c.allowed is not None
    if key == (1, 600, 70):
        assert words == 3 and all(int(out[1][0]) > 300 for out in refs.values())     # forced turns: each adds >= 1 conflict
    if key == (9, 130, 96):
        assert b == 9 and r % 32 == 0 and c.allowed is not None
        assert len({refs[False][0][e].tobytes() for e in range(b)}) == b                 # nine different envs
