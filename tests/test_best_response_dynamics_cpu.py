"""Sequential best-response RB dynamics, the part that needs no GPU: the library's exported set, the entry point's refusals, the
kernels' register budget, the refusal texts, the host-side action encoding, known answers of the reference restatement, and the
oracle's side of the GPU tests' ambiguity cap."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import best_response_dynamics_util as bu
from oracle import d2d_oracle as orc

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_brdyn_library_exports_exactly_its_header():
    from gym_d2d_amd import _native, build
    lib = _native.load_brdyn_library()
    header = (ROOT / 'include' / 'd2d_brdyn.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_brdyn.so') == declared == {'d2d_best_response_dynamics', 'd2d_brdyn_last_error'}
    assert set(_native.BRDYN_SIGNATURES) == declared
    assert len(_native.BRDYN_SIGNATURES['d2d_best_response_dynamics'][1]) == 24
    for name in declared:
        assert getattr(lib, name).restype is not None
    for const in ('BRDYN_LAW_INV_SQUARE', 'BRDYN_LAW_POWER', 'BRDYN_LAW_POW_K', 'BRDYN_MAX_RBS', 'BRDYN_MAX_ROUNDS', 'BRDYN_MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_%s (\d+)' % const, header).group(1)) == getattr(_native, const), const
    assert int(re.search(r'#define D2D_BRDYN_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    # the law ids are the sensing kernel's: sensing.fold_columns serves both
    assert (_native.BRDYN_LAW_INV_SQUARE, _native.BRDYN_LAW_POWER, _native.BRDYN_LAW_POW_K) == \
        (_native.SENSE_LAW_INV_SQUARE, _native.SENSE_LAW_POWER, _native.SENSE_LAW_POW_K)
    # built like the other side libraries, and part of the source digest
    assert build.LIBRARIES['brdyn'] == ['d2d_brdyn.hip'] and ROOT / 'include' / 'd2d_brdyn.h' in build.HEADERS
    assert build.lib_path('brdyn') == LIB_DIR / 'libd2d_brdyn.so'


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    from gym_d2d_amd.best_response_dynamics import lds_bytes
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, min_gain=3.0, max_rounds=4)

    def call(ptr=8, allowed=0, rb=8, sinr=16, rounds=24, moves=32, conv=40, **kw):
        a = dict(ok, **kw)
        _native.best_response_dynamics(ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'],
                                       a['n_rbs'], allowed, 0, a['min_gain'], a['max_rounds'], 0, rb, sinr, rounds, moves, conv)
    before = _native.brdyn_launches
    limit = str(_native.BRDYN_MAX_LDS_BYTES)
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.BRDYN_MAX_RBS + 1), 'n_rbs'), (dict(law=3), 'law'), (dict(law=-1), 'law'),
                     (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_dev=0), 'n_dev'), (dict(max_rounds=-1), 'max_rounds'),
                     (dict(max_rounds=_native.BRDYN_MAX_ROUNDS + 1), 'max_rounds'), (dict(min_gain=-0.5), 'min_gain_db'),
                     (dict(min_gain=float('nan')), 'min_gain_db'), (dict(ptr=0), 'null device pointer'),
                     (dict(rb=0), 'null device pointer'), (dict(sinr=0), 'null device pointer'), (dict(rounds=0), 'null device pointer'),
                     (dict(moves=0), 'null device pointer'), (dict(conv=0), 'null device pointer'), (dict(sinr=8), 'five arrays'),
                     (dict(conv=32), 'five arrays'), (dict(n_links=2048, n_rbs=8192, law=1), limit),
                     (dict(n_links=2048, n_rbs=512), limit), (dict(n_links=1024, n_rbs=1024, allowed=8), limit)):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    assert _native.brdyn_launches == before
    call(n_envs=0)                                                      # nothing to do: accepted, and still no launch on a device
    call(n_envs=0, max_rounds=0, min_gain=0.0)
    call(n_envs=0, n_links=512, n_rbs=256, law=1, allowed=8)            # the flagship shape fits, with a mask and the power law
    assert _native.brdyn_launches == before
    # the host's formula is the entry point's: the first shape past the limit on either side of it
    assert lds_bytes(512, 256, True, True) < 64 * 1024
    for n, r, law, allowed in ((2048, 256, 0, False), (1024, 1024, 1, True), (600, 2000, 2, False)):
        fits = lds_bytes(n, r, law != 0, allowed) <= _native.BRDYN_MAX_LDS_BYTES
        try:
            call(n_envs=0, n_links=n, n_rbs=r, law=law, pow_k=4, allowed=8 if allowed else 0)
            assert fits, (n, r)
        except _native.NativeError as e:
            assert not fits and str(lds_bytes(n, r, law != 0, allowed)) in str(e), (n, r, str(e))


def _stub_sim(route=None, shadowing=False):
    from gym_d2d_amd.path_loss_table import NATIVE
    return SimpleNamespace(path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law={'shadowing': shadowing}),
                           fixed_positions=lambda: (np.zeros(3, bool), np.zeros((3, 2))))


def test_refusal_texts_name_the_method():
    from gym_d2d_amd import best_response_dynamics as brd
    assert brd.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True, False, False]), np.array([[100.1, -20.3], [0, 0], [0, 0]]))
    texts = {'export_actions=True': brd.refusal(_stub_sim(), False),
             "'link_table'": brd.refusal(_stub_sim(route='link_table'), True),
             "'per_step'": brd.refusal(_stub_sim(route='per_step'), True),
             'ShadowingPathLoss': brd.refusal(_stub_sim(shadowing=True), True),
             'float32 cannot hold': brd.refusal(pinned, True),
             'torch path': brd.refusal(_stub_sim(), True, use_torch=False)}
    for needle, text in texts.items():
        assert needle in text and 'best_response_dynamics()' in text, (needle, text)
        assert 'sense()' not in text and 'best_rb()' not in text and 'power_control()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)


@pytest.fixture
def stub_handle(monkeypatch):
    from gym_d2d_amd import _native
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    opened = []
    monkeypatch.setattr(_native, 'load_brdyn_library', lambda: opened.append(1) or pytest.fail('libd2d_brdyn.so was opened'))
    return opened


def test_an_env_that_does_not_ask_never_opens_the_library(stub_handle):
    from gym_d2d_amd.envs import VecD2DEnv
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._brdyn is None and stub_handle == []
    # asking on the NumPy path is refused by name, at the call, still without the library
    with pytest.raises(ValueError, match=r'best_response_dynamics\(\) needs the torch path'):
        env.best_response_dynamics()
    with pytest.raises(ValueError, match=r'best_response_dynamics\(\) needs the torch path'):
        env.best_response_dynamics_actions(min_gain_db=1.0)
    assert stub_handle == [] and env._brdyn is None
    env.close()


@pytest.mark.parametrize('cue_actions', ['agent', 'traffic'])
def test_best_response_dynamics_actions_encoding_on_a_stubbed_handle(stub_handle, cue_actions):
    """6 CUEs + 4 pairs on 5 RBs: 24 CUE power levels, 21 DUE levels.  The solved RBs are hand-made; best_response_dynamics() is
    stubbed.  Decoding the actions gives the solved RBs and the current power levels back; traffic-model CUEs have no column."""
    torch = pytest.importorskip('torch')
    from gym_d2d_amd.best_response_dynamics import encode_actions
    from gym_d2d_amd.envs import VecD2DEnv
    b, cues, dues, r = 3, 6, 4, 5
    n = cues + dues
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues}, num_envs=b, use_torch=False, cue_actions=cue_actions)
    levels = np.array([24] * cues + [21] * dues)
    rng = np.random.default_rng(5)
    rb = rng.integers(0, r, (b, n)); pwr = rng.integers(0, levels, (b, n))
    rb[1, 8] = r + 2                                                    # on no RB: repeats its (out of range) action
    env.device = torch.device('cpu')
    env._t = {'rb': torch.zeros((b, n), dtype=torch.int32), 'pwr': torch.as_tensor(pwr, dtype=torch.int32)}
    planes = (torch.as_tensor(rb, dtype=torch.int32), torch.zeros((b, n)), torch.zeros(b, dtype=torch.int32),
              torch.zeros(b, dtype=torch.int32), torch.ones(b, dtype=torch.uint8))
    seen = []
    env.best_response_dynamics = lambda allowed=None, movable=None, min_gain_db=3.0, max_rounds=16, out=None, env_mask=None: \
        seen.append((allowed, movable, min_gain_db, max_rounds)) or planes
    first = 0 if cue_actions == 'agent' else cues
    a = env.best_response_dynamics_actions('mask', 'who', 1.5, 9)
    assert seen == [('mask', 'who', 1.5, 9)]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, env.num_agents) == (b, n - first)
    assert np.array_equal(a.numpy(), (rb * levels + pwr)[:, first:])
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[first:])     # the env's own decode
    assert np.array_equal(got_rb, rb[:, first:]) and np.array_equal(got_pwr, pwr[:, first:])
    a_np = encode_actions(rb, pwr, levels[first:], first)               # the function behind it: NumPy planes alike
    assert a_np.dtype == np.int32 and np.array_equal(a_np, a.numpy())
    env.close()


@pytest.fixture(scope='module')
def brdyn_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_brdyn')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_brdyn.hip'), '-save-temps', '-o', 'brdyn.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'brdyn_kernelILi(\d)EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[int(m.group(1))] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                      'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out


def test_brdyn_kernels_use_no_scratch_and_spill_nothing(brdyn_kernels):
    """law in {inverse square 0, power 1, pow-k 4}, from the resource summary alone.  The figures of the build this was written
    on: 54 VGPRs for all three kernels, 88 / 90 / 98 SGPRs; LDS is dynamic (see d2d_brdyn.hip)."""
    assert set(brdyn_kernels) == {0, 1, 4}
    for key, k in brdyn_kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0, (key, k)          # no static LDS in front of the dynamic block
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible


def test_no_atomics_in_the_brdyn_source():
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_brdyn.hip').read_text()
    code = src.split('#include', 1)[1]
    assert 'atomic' not in code.replace('no atomics', '').replace('without atomics', '')


# ------------------------------------------------------------------------------------------ known answers of the restatement
def _three_links():
    """Three DUE pairs, 10 m each, on a line; pairs 0 and 1 are 30 m apart, pair 2 is 20 km away from both."""
    cols = orc.device_columns(*orc.device_configs(0, 3)[1:])
    pos = np.array([[[0.0, 0.0], [100.0, 0.0], [110.0, 0.0], [130.0, 0.0], [140.0, 0.0], [20100.0, 0.0], [20110.0, 0.0]]])
    tx, rx = np.array([1, 3, 5]), np.array([2, 4, 6])
    return pos, tx, rx, cols, orc.PathLossSpec('log_distance', 2.1, ple=2.0)


def test_hand_computed_answers_on_three_links_and_two_rbs():
    pos, tx, rx, cols, spec = _three_links()
    pwr = np.full((1, 3), 10)
    run = lambda rb, **kw: bu.dynamics(pos, tx, rx, np.array([rb]), pwr, cols, spec, 2, **kw)
    alone = orc.step(pos, tx, rx, np.array([[0, 1, 2]]), pwr, cols, spec)['sinr_db'][0]      # everybody alone: the SNR
    # all on RB 0.  Link 0 goes first and leaves for the empty RB 1; link 1 then shares RB 0 with the far link 2 only, and what
    # RB 1 offers (link 0, 30 m away) is worse: it stays.  Link 2 gains next to nothing by joining link 0.  Round 2 is quiet.
    o = run([0, 0, 0], min_gain_db=3.0)
    assert np.array_equal(o.rb[0], [1, 0, 0]) and o.moves[0] == 1 and o.rounds[0] == 1 and o.converged[0] and not o.ambiguous[0]
    assert abs(o.sinr_db[0, 0] - alone[0]) < 1e-9 and o.sinr_db[0, 1] < alone[1] and alone[1] - o.sinr_db[0, 1] < 0.1
    # a cap of one round: the same RBs, but the round moved a link, so it is not known to be a fixed point
    capped = run([0, 0, 0], min_gain_db=3.0, max_rounds=1)
    assert np.array_equal(capped.rb[0], [1, 0, 0]) and capped.rounds[0] == 1 and not capped.converged[0]
    zero = run([0, 0, 0], max_rounds=0)
    assert np.array_equal(zero.rb[0], [0, 0, 0]) and zero.rounds[0] == 0 and zero.moves[0] == 0 and not zero.converged[0]
    # only link 1 may move: it is the one that leaves
    o = run([0, 0, 0], movable=np.array([False, True, False]))
    assert np.array_equal(o.rb[0], [0, 1, 0]) and o.moves[0] == 1 and o.converged[0]
    # link 0 may only use RB 0: it stays, link 1 leaves instead; a link with no allowed RB and a link on no RB never move
    allowed = np.array([[True, False], [True, True], [True, True]])
    o = run([0, 0, 0], allowed=allowed)
    assert np.array_equal(o.rb[0], [0, 1, 0])
    o = run([0, 0, 0], allowed=np.array([[False, False], [False, False], [True, True]]))
    assert np.array_equal(o.rb[0], [0, 0, 0]) and o.moves[0] == 0 and o.rounds[0] == 0 and o.converged[0]
    o = run([7, 0, 0])
    assert np.array_equal(o.rb[0], [7, 0, 0]) and np.isnan(o.sinr_db[0, 0]) and o.moves[0] == 0   # and it interferes with nobody:
    assert abs(o.sinr_db[0, 1] - run([1, 0, 0]).sinr_db[0, 1]) < 1e-12
    # already apart: the near links' gains are 0 exactly, and 0 is not above a hysteresis of 0 (the far link is left out: to it
    # the two RBs are the same within the bar, which is what the ambiguity rule is for)
    o = run([1, 0, 1], min_gain_db=0.0, movable=np.array([True, True, False]))
    assert o.moves[0] == 0 and o.rounds[0] == 0 and o.converged[0] and not o.ambiguous[0]
    assert run([1, 0, 1], min_gain_db=0.0).ambiguous[0]
    # the hysteresis: link 0 gains this much by leaving link 1 for the far link 2; a min_gain_db above that keeps it
    shared = orc.step(pos, tx, rx, np.array([[0, 0, 1]]), pwr, cols, spec)['sinr_db'][0]
    gain = orc.step(pos, tx, rx, np.array([[1, 0, 1]]), pwr, cols, spec)['sinr_db'][0, 0] - shared[0]
    assert gain > 3.0
    assert run([0, 0, 1], min_gain_db=gain + 0.5, movable=np.array([True, False, False])).moves[0] == 0
    assert run([0, 0, 1], min_gain_db=gain - 0.5, movable=np.array([True, False, False])).moves[0] == 1
    assert run([0, 0, 1], min_gain_db=gain + 1e-7, movable=np.array([True, False, False])).ambiguous[0]


# ------------------------------------------------------------------------------------------ the ambiguity cap of the GPU cases
@pytest.mark.parametrize('name', list(bu.CASES))
def test_oracle_ambiguity_of_the_gpu_cases_stays_inside_the_cap(name):
    """The seeds of the GPU test's oracle comparison, on the oracle alone: at most 25 % of a case's envs are ambiguous
    (best_response_dynamics_util), and the cases exercise what they are there for."""
    from gym_d2d_amd import _native
    from gym_d2d_amd.best_response_dynamics import lds_bytes
    c, o = bu.make_case(name), bu.oracle_side(name)
    share = float(o.ambiguous.mean())
    lds = lds_bytes(c.n, c.r, c.law != 'ld2', False)
    print(f'{name}: {share:.2%} of {c.b} envs ambiguous; rounds {o.rounds.min()}..{o.rounds.max()}, moves {o.moves.min()}..'
          f'{o.moves.max()}, converged {o.converged.mean():.0%}; {lds} bytes of LDS; moves into each RB block '
          f'{np.bincount(bu.rb_blocks(c.r), weights=o.dest).astype(int).tolist()}, {int(o.dest[256:].sum())} of them at r >= 256, '
          f'{int(o.moved[1024:].sum())} by links j >= 1024')
    assert o.ambiguous.shape == (c.b,) and share <= bu.CAP
    assert (~o.ambiguous).sum() >= 3                                    # a small batch still compares something
    assert o.on_rb.all() and np.isfinite(o.sinr_db).all()
    assert (o.moves > 0).any() and (o.rounds <= c.max_rounds).all() and ((o.rounds == c.max_rounds) <= ~o.converged).all()
    assert (o.moves >= o.rounds).all() and ((o.rb != c.rb).sum(axis=1) <= o.moves).all()
    assert o.dest.sum() == o.moves.sum() == o.moved.sum()
    if name not in ('n20_r64', 'n320_r2500'):                           # (those two: mostly empty RBs, one round settles it)
        assert o.rounds.max() >= 2                                      # later links answer earlier moves
    # what the multi-wave and large-LDS cases are there for, on the reference alone
    assert lds <= _native.BRDYN_MAX_LDS_BYTES
    if c.r > 64:
        assert bu.covers(o.dest, c.r)                                   # every wave holds a winner, both RBs of a lane past 256
    if name in ('n2048_r256', 'n320_r2500'):
        assert lds > 64 * 1024
    if c.n > 1024:
        assert o.moved[1024:].sum() > 0 and (c.movable is None or not o.moved[~c.movable].any())
