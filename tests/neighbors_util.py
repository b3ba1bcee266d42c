"""The oracle's side of the neighbour-graph tests (test_neighbors_cpu.py, test_gpu_neighbors.py), in float64.

Index order everywhere: [b, i, j] - receiver link i first, transmitter link j last (orc.pair_path_loss_db is [b, j, i])."""
import numpy as np

from oracle import d2d_oracle as orc

CAP = 0.05                 # the largest share of a case's index entries the near-tie rule may leave out


def coupling_ref(pos, link_tx, link_rx, cols, spec):
    """ref[b, i, j] = eirp_off_db[tx_j] - PL(tx_j -> rx_i)."""
    tx, rx = np.asarray(link_tx, dtype=np.int64), np.asarray(link_rx, dtype=np.int64)
    pl = orc.pair_path_loss_db(spec, np.asarray(pos, dtype=np.float64), tx, rx, cols)                # [b, j, i]
    return np.ascontiguousarray((np.asarray(cols.eirp_off_db)[tx][None, :, None] - pl).transpose(0, 2, 1))


def ranked(ref, k):
    """(idx [B, N, k], values [B, N, k], comparable bool [B, N, k]) of the oracle: a stable descending sort of each row with the
    diagonal removed (equal values in ascending j).  An index entry is comparable when the oracle's gaps to the ranks on both sides of
    it (rank k + 1 included) are either exactly 0 - a true tie, where the ascending-j rule must hold exactly - or above
    margin = 2e-5 * max(1, max |ref|) dB: twice what the 1e-5 bar allows two float32 results to differ by."""
    b, n, _ = ref.shape
    assert 1 <= k <= n - 1
    margin = 2e-5 * max(1.0, float(np.abs(ref).max()))
    c = ref.copy()
    c[:, np.arange(n), np.arange(n)] = -np.inf
    order = np.argsort(-c, axis=2, kind='stable')[:, :, :n - 1]              # the diagonal sorts last: dropped
    vals = np.take_along_axis(c, order, axis=2)
    gap = vals[:, :, :-1] - vals[:, :, 1:]                                   # gap[m]: between ranks m and m + 1
    fine = (gap == 0.0) | (gap > margin)
    fine = np.concatenate([np.ones((b, n, 1), bool), fine, np.ones((b, n, 1), bool)], axis=2)    # nothing above rank 0 / below the last
    comparable = fine[:, :, :k] & fine[:, :, 1:k + 1]
    return order[:, :, :k], vals[:, :, :k], comparable


def check_indices(got_idx, ref, k):
    """Assert the index rule of `ranked` on got_idx [B, N, k]; returns (share left out, share of exact ties among the gaps)."""
    idx, vals, comparable = ranked(ref, k)
    left_out = 1.0 - float(comparable.mean())
    assert left_out <= CAP, f'{left_out:.2%} of the index entries are near ties: above the {CAP:.0%} cap'
    wrong = comparable & (np.asarray(got_idx, dtype=np.int64) != idx)
    assert not wrong.any(), f'{int(wrong.sum())} comparable index entries differ, first at {np.argwhere(wrong)[0].tolist()}'
    ties = float((vals[:, :, :-1] == vals[:, :, 1:]).mean()) if k > 1 else 0.0
    return left_out, ties


def check_sets(got_idx, n):
    """Every row: in range, free of duplicates, free of the row's own link."""
    got = np.asarray(got_idx, dtype=np.int64)
    assert got.min() >= 0 and got.max() < n
    s = np.sort(got, axis=2)
    assert (s[:, :, 1:] != s[:, :, :-1]).all()
    assert (got != np.arange(got.shape[1])[None, :, None]).all()


def gather_obs(idx, coupling_db, rb, pwr, sinr_db, snr_db):
    """[B, N, 4 (k + 1)]: own (rb, pwr, sinr, snr), then per neighbour (coupling, rb_j, pwr_j, sinr_j)."""
    b, n, k = idx.shape
    out = np.empty((b, n, k + 1, 4), dtype=np.float64)
    out[:, :, 0] = np.stack([rb, pwr, sinr_db, snr_db], axis=-1)
    env = np.arange(b)[:, None, None]
    out[:, :, 1:, 0] = coupling_db
    out[:, :, 1:, 1] = rb[env, idx]
    out[:, :, 1:, 2] = pwr[env, idx]
    out[:, :, 1:, 3] = sinr_db[env, idx]
    return out.reshape(b, n, 4 * (k + 1))
