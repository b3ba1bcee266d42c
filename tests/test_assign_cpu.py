"""Optimal one-to-one RB matching, the part that needs no GPU: the library's exported set and its place in the build, the entry
points' refusals, the kernels' register budget, the refusal texts, the separability identity of the weight planes against
evaluate_util.evaluate_ref, the restatement of the matching against brute force and scipy, and the reference's side of the GPU
tests' threshold cap."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import assign_util as asu
import evaluate_util as evu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_assign_library_exports_exactly_its_header():
    from gym_d2d_amd import _native, build
    lib = _native.load_assign_library()
    assert _native.side_library('assign') is lib
    header = (ROOT / 'include' / 'd2d_assign.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_assign.so') == declared == {'d2d_assign_weights', 'd2d_assign_solve', 'd2d_assign_last_error'}
    assert set(_native.ASSIGN_SIGNATURES) == declared and _native.SOLVERS == {'assign': _native.ASSIGN_SIGNATURES}
    assert len(_native.ASSIGN_SIGNATURES['d2d_assign_weights'][1]) == 21 and len(_native.ASSIGN_SIGNATURES['d2d_assign_solve'][1]) == 8
    for symbol, (res, args) in _native.ASSIGN_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == args
    for const in ('ASSIGN_LAW_INV_SQUARE', 'ASSIGN_LAW_POWER', 'ASSIGN_LAW_POW_K', 'ASSIGN_OBJECTIVE_TOTAL', 'ASSIGN_OBJECTIVE_OWN',
                  'ASSIGN_MAX_RBS', 'ASSIGN_MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_%s (\d+)' % const, header).group(1)) == getattr(_native, const), const
    assert int(re.search(r'#define D2D_ASSIGN_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    assert (_native.ASSIGN_LAW_INV_SQUARE, _native.ASSIGN_LAW_POWER, _native.ASSIGN_LAW_POW_K, _native.ASSIGN_MAX_RBS) == \
        (_native.SENSE_LAW_INV_SQUARE, _native.SENSE_LAW_POWER, _native.SENSE_LAW_POW_K, _native.SENSE_MAX_RBS)
    # built, stamped and found like the others; the evaluate library keeps its two symbols
    assert build.SOLVERS == {'assign': ['d2d_assign.hip']} and list(build.BUILT) == list(build.LIBRARIES) + ['assign']
    assert ROOT / 'include' / 'd2d_assign.h' in build.HEADERS and build.CSRC / 'd2d_assign.hip' in build.digest_files()
    assert build.lib_path('assign') == LIB_DIR / 'libd2d_assign.so' == _native.side_path('assign')
    assert _exports('libd2d_evaluate.so') == set(_native.EVALUATE_SIGNATURES)


def test_a_missing_assign_library_is_rebuilt(tmp_path, monkeypatch):
    from gym_d2d_amd import build
    assert build.solvers_built() and not build.solvers_built(tmp_path)
    build.lib_path('assign', tmp_path).touch()
    assert build.solvers_built(tmp_path)
    # up to date by the stamp and the twelve, the solver missing: build() does not return early but reaches for the compiler
    monkeypatch.setattr(build, 'solvers_built', lambda lib_dir=build.LIB_DIR: False)
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest())
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, n_movable=1, objective=0)

    def weights(ptr=8, links=8, allowed=0, out=8, harm=16, **kw):
        a = dict(ok, **kw)
        _native.assign_weights(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'],
                               a['n_rbs'], links, a['n_movable'], allowed, a['objective'], out, harm)
    before = _native.assign_weights_launches, _native.assign_solve_launches
    big = asu.lds_bytes(2048, 8192, True)
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.ASSIGN_MAX_RBS + 1), 'n_rbs'), (dict(n_movable=0), 'n_movable'), (dict(n_movable=3), 'n_movable'),
                     (dict(law=3), 'law'), (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_dev=0), 'n_dev'), (dict(objective=2), 'unknown objective'), (dict(objective=-1), 'unknown objective'),
                     (dict(ptr=0), 'null device pointer'), (dict(links=0), 'null device pointer'), (dict(out=0), 'null device pointer'),
                     (dict(harm=8), 'weights and harm must be two planes'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=8192, law=1), f'n_links and n_rbs need {big} bytes of LDS, more than the 163840'),
                     (dict(n_links=2048, n_rbs=8192, law=1, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            weights(**kw)
    for kw in (dict(), dict(harm=0), dict(allowed=8), dict(n_links=2048, n_rbs=64, n_movable=2048), dict(objective=1)):
        weights(n_envs=0, **kw)                                        # nothing to do: accepted, and no launch on a device

    def solve(w=8, col=8, value=8, feasible=8, n_envs=2, m=2, r=3):
        _native.assign_solve(w, n_envs, m, r, col, value, feasible)
    big = asu.solve_lds_bytes(4096, 8192)
    for kw, text in ((dict(m=4, r=3), 'n_rows = 4 rows cannot be matched one-to-one to n_cols = 3 columns'), (dict(m=0), 'n_rows'),
                     (dict(r=0), 'n_cols'), (dict(r=_native.ASSIGN_MAX_RBS + 1), 'n_cols'), (dict(n_envs=-1), 'n_envs'),
                     (dict(w=0), 'null device pointer'), (dict(col=0), 'null device pointer'), (dict(value=0), 'null device pointer'),
                     (dict(feasible=0), 'null device pointer'),
                     (dict(m=4096, r=8192), f'n_rows and n_cols need {big} bytes of LDS, more than the 163840'),
                     (dict(m=4096, r=8192, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            solve(**kw)
    solve(n_envs=0)
    solve(n_envs=0, m=2048, r=2048)
    assert (_native.assign_weights_launches, _native.assign_solve_launches) == before


def test_lds_bytes_are_the_headers_formulas():
    from gym_d2d_amd import _native, assignment
    for n, r in ((1, 1), (3, 4), (63, 64), (257, 259), (1000, 8), (2048, 8192), (260, 4000)):
        for power_law in (False, True):
            assert assignment.lds_bytes(n, r, power_law) == asu.lds_bytes(n, r, power_law)
    for m, r in ((1, 1), (3, 4), (64, 65), (257, 257), (5, 4000), (2048, 8192)):
        assert assignment.solve_lds_bytes(m, r) == asu.solve_lds_bytes(m, r)
    # which side of the 64 KiB branch the GPU cases stand on: one weights case and one matching (5 x 4000) past it; the link limit
    # with a power law on few RBs fits, and so does a square matching of 4096 rows
    sizes = [asu.lds_bytes(cues + dues, r, law != 'ld2') for cues, dues, r, law in asu.WEIGHT_CASES]
    assert max(sizes) > 64 * 1024 and sorted(sizes)[-2] <= 64 * 1024
    sizes = sorted(asu.solve_lds_bytes(m, r) for m, r in asu.SOLVE_SHAPES)
    assert sizes[-1] > 64 * 1024 >= sizes[-2]
    assert asu.lds_bytes(2048, 64, True) <= _native.ASSIGN_MAX_LDS_BYTES < asu.lds_bytes(2048, 8192, False)
    assert asu.solve_lds_bytes(4096, 4096) <= _native.ASSIGN_MAX_LDS_BYTES < asu.solve_lds_bytes(8192, 8192)
    assert asu.lds_bytes(512, 256, True) < 48 * 1024                  # the benchmark shape fits three times into a CU's LDS


def _stub_sim(route=None, shadowing=False):
    from gym_d2d_amd.path_loss_table import NATIVE
    return SimpleNamespace(path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law={'shadowing': shadowing}),
                           fixed_positions=lambda: (np.zeros(3, bool), np.zeros((3, 2))))


def test_refusal_texts_are_evaluates_under_this_name():
    from gym_d2d_amd import assignment, evaluate
    assert assignment.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True, False, False]), np.array([[100.1, -20.3], [0, 0], [0, 0]]))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), 'ShadowingPathLoss': (_stub_sim(shadowing=True), True),
             'float32 cannot hold': (pinned, True)}
    texts = {needle: assignment.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = assignment.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and 'assign_rbs()' in text and 'evaluate()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle in ("'link_table'", 'ShadowingPathLoss', 'float32 cannot hold'):        # evaluate()'s words, this API's name
        assert texts[needle] == evaluate.refusal(*stubs[needle]).replace('evaluate()', 'assign_rbs()')


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    opened = []
    monkeypatch.setattr(_native, 'load_assign_library', lambda: opened.append(1) or pytest.fail('libd2d_assign.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._assign is None and opened == []
    for call in (env.assignment_weights, env.assign_rbs, env.assign_rbs_actions, lambda: env.solve_assignment(None)):
        with pytest.raises(ValueError, match=r'assign_rbs\(\) needs the torch path'):
            call()
    assert opened == []
    env.close()


@pytest.fixture(scope='module')
def assign_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_assign')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_assign.hip'), '-save-temps', '-o', 'assign.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'(assign_weights_kernelILi\dELi\dEE|assign_solve_kernelILi\d+EE)', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[m.group(1)] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                 'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out, asm


def test_assign_kernels_use_no_scratch_no_atomics_and_spill_nothing(assign_kernels):
    """Six weights kernels (law in {0, 1, 4} x objective in {0, 1}) and two matching kernels (64 and 256 threads).  The figures of
    the build this was written on: 60 - 64 VGPRs for the weights kernels, 60 for both matching kernels; LDS is dynamic."""
    kernels, asm = assign_kernels
    assert len(kernels) == 8 and {'assign_solve_kernelILi64EE', 'assign_solve_kernelILi256EE'} <= set(kernels)
    for key, k in kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0, (key, k)
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_assign.hip').read_text()
    code = src.split('#include', 1)[1]
    assert 'atomic' not in code and 'nontemporal' not in code
    assert not re.search(r'^\s*(global|flat|buffer|ds)_(atomic|add_f|add_rtn|cmpst)', asm, flags=re.M)
    assert 'scratch_' not in asm


# ------------------------------------------------------------------------------------------ the separability identity
@pytest.mark.parametrize('cues,dues,r,law', [(3, 3, 4, 'ld35'), (13, 50, 64, 'mixed'), (57, 200, 200, 'ld2')])
def test_total_capacity_separates_over_one_to_one_placements(cues, dues, r, law):
    """G(placement) = G(background) + sum over a of (own - harm)[a, r_a] for injective a -> r_a, at 1e-9 relative, against
    evaluate_util.evaluate_ref on complete assignments: a random injective placement, the optimum of the 'total' plane and the
    optimum of the 'own' plane per env - and it FAILS for a placement that shares an RB, which is why one-to-one makes it exact."""
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues)
    own, harm, near = asu.weights_ref(c, links)
    w = own - harm
    assert (harm >= 0).all() and (own >= 0).all()
    m = len(links)
    rng = np.random.default_rng(3)
    placements = {'random': np.stack([rng.permutation(r)[:m] for _ in range(c['b'])]),
                  'total': np.stack([asu.solve_ref(w[e].astype(np.float32))[0] for e in range(c['b'])]),
                  'own': np.stack([asu.solve_ref(own[e].astype(np.float32))[0] for e in range(c['b'])])}
    rbs = np.stack([asu.background_candidate(c, links)] + [asu.placement_candidate(c, links, p) for p in placements.values()], axis=1)
    pwr = np.repeat(np.asarray(c['pwr'])[:, None, :], rbs.shape[1], axis=1)
    _, cap, total = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], rbs, pwr, c, r)
    # the background-only sub-case: the movable links on rb -1 interfere with nobody, and their own (interference-free) capacities
    # there are no part of it
    background = np.delete(cap[:, 0], links, axis=1).sum(axis=1)
    for q, (name, cols) in enumerate(placements.items(), start=1):
        assert all(len(set(row)) == m for row in cols.tolist())
        parts = background + w[np.arange(c['b'])[:, None], np.arange(m)[None, :], cols].sum(axis=1)
        err = float(np.abs(parts / total[:, q] - 1.0).max())
        print(f'{cues} + {dues} links, {r} RBs, {law}, {name}: identity holds to {err:.2e}; {(w < 0).mean():.1%} of the weights negative, '
              f'{near.mean():.2%} near a threshold')
        assert err <= 1e-9
    assert (total[:, 2] >= total[:, 1] - 1e-9 * total[:, 1]).all()       # the optimum is no worse than the random placement
    # two movable links on ONE RB: the identity is off by their mutual interference
    shared = placements['random'].copy()
    shared[:, 1] = shared[:, 0]
    _, _, t2 = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], asu.placement_candidate(c, links, shared)[:, None], pwr[:, :1], c, r)
    parts = background + w[np.arange(c['b'])[:, None], np.arange(m)[None, :], shared].sum(axis=1)
    assert (parts > t2[:, 0] * (1.0 + 1e-9)).all()


# ------------------------------------------------------------------------------------------ the matching's restatement
def _small_matrices():
    rng = np.random.default_rng(12)
    for q in range(400):
        m = int(rng.integers(1, 6))
        r = int(rng.integers(m, 7))
        kind = q % 4
        if kind == 0:
            w = rng.integers(0, 4, (m, r)).astype(np.float32)                # ties
        elif kind == 1:
            w = rng.normal(0.0, 5.0, (m, r)).astype(np.float32)
        else:
            w = (rng.normal(0.0, 5.0, (m, r)) if kind == 2 else rng.integers(-2, 3, (m, r))).astype(np.float32)
            w[rng.random((m, r)) < 0.4] = -np.inf                            # 40 % forbidden: some have no matching
            if q % 8 == 2:
                w[rng.integers(m), rng.integers(r)] = np.nan
        yield w


def test_restatement_against_brute_force():
    feasible = infeasible = 0
    for w in _small_matrices():
        col, value, ok = asu.solve_ref(w)
        best = asu.brute_force(w)
        assert (best is not None) == bool(ok), w
        if not ok:
            infeasible += 1
            assert (col == -1).all() and value == 0.0
            continue
        feasible += 1
        m = w.shape[0]
        assert len(set(col.tolist())) == m and np.isfinite(w[np.arange(m), col]).all()
        got = float(w[np.arange(m), col].astype(np.float64).sum())
        assert abs(got - best) <= 1e-9 * max(abs(best), 1.0), (w, col, got, best)
        assert value == np.float32(got)
    print(f'{feasible} feasible and {infeasible} infeasible matrices, 0 mismatches')
    assert feasible > 200 and infeasible > 20


def test_restatement_against_scipy():
    opt = pytest.importorskip('scipy.optimize')
    for m, r in ((64, 65), (200, 259), (100, 100)):
        w = asu.solve_matrix(m, r) if (m, r) != (100, 100) else np.random.default_rng(2).integers(0, 4, (100, 100)).astype(np.float32)
        col, value, ok = asu.solve_ref(w)
        cost = np.where(np.isfinite(w), -w.astype(np.float64), 1e9)
        rows, cols = opt.linear_sum_assignment(cost)
        want = float(w[rows, cols].astype(np.float64).sum())
        got = float(w[np.arange(m), col].astype(np.float64).sum())
        print(f'{m} x {r}: restatement {got:.6f}, scipy {want:.6f}')
        assert ok and abs(got - want) <= 1e-9 * abs(want)


def test_the_chain_matrix_passes_through_every_row():
    w = asu.chain_matrix(65)
    col, value, ok = asu.solve_ref(w)
    assert ok and np.array_equal(col, np.r_[np.arange(1, 65), 0]) and value == np.float32(65.0)


# ------------------------------------------------------------------------------------------ the GPU cases, reference side
def _share(own, harm, near, name):
    left_out = float(near.mean())
    print(f'{name}: {left_out:.2%} of {near.size} entries near a threshold; {(own - harm < 0).mean():.1%} of the weights negative, '
          f'{(own > 0).mean():.1%} of the own capacities above the sensitivity')
    assert left_out <= asu.THRESHOLD_CAP
    assert np.isfinite(own).all() and np.isfinite(harm).all() and (harm >= 0).all() and (own >= 0).all()


@pytest.mark.parametrize('cues,dues,r,law', asu.WEIGHT_CASES)
def test_threshold_share_of_the_gpu_cases_stays_inside_the_cap(cues, dues, r, law):
    """The seeds of the GPU test's comparison, on the reference alone: at most 1 % of a case's entries are near a threshold.  harm
    is 0.0 exactly on the RBs without background members, and positive somewhere."""
    c = asu.case(cues, dues, r, law)
    own, harm, near = asu.case_ref(cues, dues, r, law)
    assert own.shape == harm.shape == near.shape == (asu.B, dues, r)
    _share(own, harm, near, f'{cues} + {dues} links, {r} RBs, {law}')
    rb = np.asarray(c['rb'])[:, :cues]
    for e in range(asu.B):
        empty = np.setdiff1d(np.arange(r), rb[e][(rb[e] >= 0) & (rb[e] < r)])
        assert (harm[e][:, empty] == 0.0).all()
    assert (harm > 0).any() and (own > 0).any()


def test_threshold_share_of_the_scattered_case_stays_inside_the_cap():
    c = asu.case(*asu.SCATTERED)
    links, allowed = asu.scattered_movable(c)
    own, harm, near = asu.scattered_ref()
    _share(own, harm, near, 'scattered movable')
    assert (links < 13).any() and (links >= 13).any() and 0.6 < allowed.mean() < 0.8 and own.shape == (asu.B, len(links), c['r'])
