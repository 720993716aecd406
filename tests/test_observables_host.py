"""Host side of the jet-observable evaluation (observables.py): mode parsing with the reference's semantics
(evaluation/eval.py:238-313, 413-430), the histogram / KL summary (eval.py:598-718) on G17's fixed lists, and the batch-drop
rules of MultHist.append (eval.py:314-379) on synthetic kernel records.  No GPU."""
import os

import numpy as np
import pytest

from conftest import load_pkg

obs = load_pkg().observables
L = load_pkg()._lib
MODES = ['max', 'min', 'mean', 'nnz', 'meannnz', 'E', 'E_1', 'E_2', 'E_5', 'E_10', 'E_30', 'R_12', 'R_25', 'deltaR_12', 'deltaR_13',
         'FWM_1_5', 'FWM_2_10', 'FWM_1_30', 'jetmass', 'hitogram', 'meanimg']


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(os.path.join(golden_dir, "G17_observables.npz"))


def test_mode_parsing_matches_multhist():
    s = obs.parse_mode('E_30')
    assert (s.kind, s.nums, s.power, s.display_ratio, s.args) == ('E_n', 4, 0.5, 0.98, (30,))
    s = obs.parse_mode('corr_R_25_lr')
    assert (s.base, s.kind, s.power, s.args) == ('R_25', 'R', 0.5, (2, 5))
    s = obs.parse_mode('deltaR_13')
    assert (s.kind, s.power, s.args) == ('deltaR', 1.0, (1, 3))
    s = obs.parse_mode('ratio_FWM_2_10')
    assert (s.base, s.kind, s.nums, s.args) == ('FWM_2_10', 'FWM', 4, (2, 10))
    for mode, nums in (('max', 3), ('min', 3), ('mean', 2), ('nnz', 4), ('meannnz', 4), ('E', 2), ('jetmass', 4), ('hitogram', 2),
                       ('meanimg', 2)):
        assert obs.parse_mode(mode).nums == nums, mode
    assert obs.parse_mode('E').power == 0.5 and obs.parse_mode('meannnz').display_ratio == 0.95
    assert obs.top_k_needed(obs.parse_modes(['E_1', 'FWM_1_30', 'deltaR_12'])) == 30
    assert obs.top_k_needed(obs.parse_modes(['max'])) == 9
    assert obs.fwm_pairs(obs.parse_modes(['FWM_1_5', 'corr_FWM_1_5', 'FWM_2_10'])) == [(1, 5), (2, 10)]


@pytest.mark.parametrize("mode,pkg", [("wmass", "pyjet"), ("nsubj_2_1", "pyjet"), ("w_pf", "energyflow"), ("C_0_2", "energyflow")])
def test_clustering_modes_raise(mode, pkg):
    with pytest.raises(NotImplementedError, match=pkg):
        obs.parse_mode(mode)


def test_unknown_modes_raise():
    for mode in ('foo', 'E_65', 'FWM_1_65'):
        with pytest.raises(ValueError):
            obs.parse_mode(mode)


def _lists(g17, tag, modes):
    out = {}
    for m in modes:
        if m in obs.MAP_MODES:
            continue
        out[m] = [g17[f"{tag}.list.{m}.{i}"] for i in range(obs.parse_mode(m).nums)]
    return out


@pytest.mark.parametrize("tag", ["jets80", "jets40"])
@pytest.mark.parametrize("nth", ["hr", "lr", "both"])
def test_kl_summary_on_golden_lists(g17, tag, nth):
    specs = obs.parse_modes(MODES)
    maps = {m: [g17[f"{tag}.map.{m}.0"], g17[f"{tag}.map.{m}.1"]] for m in obs.MAP_MODES}
    total, kld, hists = obs.summarize(specs, _lists(g17, tag, MODES), maps, bins=30, nth_jet_eval_mode=nth)
    np.testing.assert_array_equal(np.array(total), g17[f"{tag}.total_kld.{nth}"])
    ref = {k.split('.')[-1]: float(g17[k]) for k in g17.files if k.startswith(f"{tag}.kld.{nth}.")}
    assert kld == ref
    if nth == "hr":
        for m, h in hists.items():
            for i, (e, be) in enumerate(zip(h['entries'], h['binedges'])):
                np.testing.assert_array_equal(e, g17[f"{tag}.hist.{m}.{i}"], err_msg=m)
                np.testing.assert_array_equal(be, g17[f"{tag}.edges.{m}.{i}"], err_msg=m)


def _records(values, sizes, topv, topi, ties, H=4, W=4):
    n = sum(sizes)
    st = np.zeros((n, L.EVAL_NSTAT))
    st[:, L.EVAL_NAN] = [1.0 if np.isnan(v) else 0.0 for v in values]
    st[:, L.EVAL_MAX] = np.nan_to_num(values)
    return dict(stats=st, topv=np.asarray(topv, np.float32), topi=np.asarray(topi, np.int32), ties=np.asarray(ties, np.int32),
                fwm=np.zeros((n, 1)), sizes=sizes, H=H, W=W, pairs=[(1, 2)], values=None)


def test_batch_drop_rules():
    K = 9
    topv = np.tile(np.arange(K, 0, -1, dtype=np.float32), (6, 1))
    topi = np.tile(np.arange(K), (6, 1))
    ties = np.ones((6, K))
    values = [1.0, 2.0, np.nan, 4.0, 5.0, 6.0]
    sizes = [2, 2, 1, 1]                         # batch 1 holds a NaN; batches 2, 3 hold one image each
    rec = _records(values, sizes, topv, topi, ties)
    mx = obs.parse_mode('max')
    assert obs.extract(rec, mx).tolist() == [1.0, 2.0, 5.0, 6.0]
    assert obs.extract(rec, mx, reference_quirks=False).tolist() == [1.0, 2.0, 4.0, 5.0, 6.0]
    for m in ('E_1', 'R_12', 'deltaR_12', 'FWM_1_2', 'jetmass'):
        assert len(obs.extract(rec, obs.parse_mode(m))) == 2, m               # batch of one: nothing
        assert len(obs.extract(rec, obs.parse_mode(m), reference_quirks=False)) == 5, m
    # R_nm with a zero m-th value in one image drops its whole batch
    topv2 = topv.copy()
    topv2[1, 1] = 0
    rec = _records([1.0] * 6, [2, 2, 2], topv2, topi, ties)
    assert len(obs.extract(rec, obs.parse_mode('R_12'))) == 4
    r = obs.extract(rec, obs.parse_mode('R_12'), reference_quirks=False)
    assert len(r) == 6 and np.isinf(r[1])
    # deltaR_nm with a tied n-th or m-th value drops its batch (np.where finds two positions); R_nm is not affected
    ties2 = ties.copy()
    ties2[4, 2] = 2
    rec = _records([1.0] * 6, [2, 2, 2], topv, topi, ties2)
    assert len(obs.extract(rec, obs.parse_mode('deltaR_13'))) == 4
    assert len(obs.extract(rec, obs.parse_mode('deltaR_12'))) == 6
    assert len(obs.extract(rec, obs.parse_mode('deltaR_13'), reference_quirks=False)) == 6


def test_deltar_uses_reference_bin_centres():
    """eval.py:195 takes bins = arr.shape[1] = 1 of the [B, 1, H, W] batch: positions (r, c) sit at (2r, 2c)."""
    topv = np.tile(np.arange(9, 0, -1, dtype=np.float32), (2, 1))
    topi = np.tile(np.arange(9), (2, 1))
    topi[0, :2] = [0, 3 * 4 + 4 - 1]             # (0, 0) and (3, 3) in a 4x4 image
    rec = _records([1.0, 1.0], [2], topv, topi, np.ones((2, 9)))
    d = obs.extract(rec, obs.parse_mode('deltaR_12'))
    assert d.dtype == np.float64 and d[0] == np.sqrt(2 * 6.0 ** 2)


def test_meannnz_int_zero_promotes_like_numpy():
    rec = _records([1.0, 1.0], [2], np.ones((2, 9)), np.zeros((2, 9)), np.ones((2, 9)))
    rec['stats'][0, L.EVAL_NNZ], rec['stats'][0, L.EVAL_NNZ_SUM] = 2, 3.0
    v = obs.extract(rec, obs.parse_mode('meannnz'))
    ref = np.array([np.float32(1.5), 0])         # what np.array of the reference's list gives
    assert v.dtype == ref.dtype and v.tolist() == ref.tolist()
