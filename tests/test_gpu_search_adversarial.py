"""The 2 eps slack of the two-precision search attacked on the GPU: rounding-adversarial corpora (search_adversarial_util.py;
tests/test_search_adversarial_fixture.py proves on the CPU what they are) whose true top-k rows the fp16 filter under-estimates
against their competitors by 30-35 % of the kernel's own 2 eps.  Ids and scores must be bit-identical to the fmaf-chain
oracle; a slack about three times too small at ANY of its sites -- the threshold a prune hands to the insertion test, the
prune itself, the rescore band, a threshold taken over from a sibling split -- loses victims here.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import search_adversarial_util as A
from test_gpu_search import _diag  # diag_<name>.json on a mismatch, beside the other search tests' diagnostics

pytestmark = pytest.mark.gpu

@pytest.fixture(autouse=True)
def _knobs_follow_the_environment():
    """The library reads its ANCE_* knobs once per process; the tests below change them with monkeypatch.  This fixture is
    set up before monkeypatch, so its teardown runs after the environment has been restored."""
    yield
    from ance_amd import _lib
    _lib.reload_env()


@functools.lru_cache(maxsize=None)
def _oracle(key, split_case=False):
    """(D, I) of the fmaf-chain oracle for a fixture, computed once (on the distinct queries of a tiled block)."""
    from oracle import search_ref
    F = A.build(**A.SPLIT_CASES[key]) if split_case else A.fixture(key)
    u = F.n_unique
    D, I = search_ref.flat_ip_topk_chain(F.x, F.q[:u], F.k)
    for r in np.flatnonzero(F.tie_sign[:u]):  # (the CPU self-check proves it; a fixture that drifted must not pass here)
        assert np.array_equal(I[r], F.victims if F.tie_sign[r] > 0 else F.neg_victims)
    return D, I


def _index(F):
    from ance_amd import _lib
    from ance_amd.index import FlatIPIndex
    _lib.reload_env()
    idx = FlatIPIndex(F.d)
    idx.add(np.array(F.x))  # (the cached fixture is read-only)
    return idx


def _check_exact(name, F, Do, Io, idx=None, **kw):
    import torch
    idx = idx if idx is not None else _index(F)
    D, I = idx.search_device(torch.from_numpy(np.array(F.q)).cuda(), F.k, **kw)
    torch.cuda.synchronize()
    D, I = D.cpu().numpy(), I.cpu().numpy()
    u = Do.shape[0]
    rep = np.arange(len(F.q)) % u  # row of the oracle's answer for every query of a tiled block
    bad = np.argwhere((I != Io[rep]) | (D != Do[rep]))
    if len(bad):
        r = int(bad[0][0])
        lost = np.setdiff1d(Io[rep[r]], I[r])
        _diag(name, n=F.n, nq=len(F.q), k=F.k, n_bad=int(len(bad)), bad_queries=np.unique(bad[:, 0])[:64], first_bad=bad[0],
              tie_sign=int(F.tie_sign[r]), n_lost=int(len(lost)), lost_roles=F.role[lost][:32], I=I[r], Io=Io[rep[r]],
              D=D[r].astype(float), Do=Do[rep[r]].astype(float))
    assert np.array_equal(I, Io[rep]), "%s: ids differ from the oracle (see diag_%s.json)" % (name, name)
    assert np.array_equal(D, Do[rep]), "%s: scores differ bitwise from the fmaf-chain oracle" % name
    return idx


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_adversarial_rows_bit_exact(name):
    """Every (d, n, k) x placement x fixture kind: impostors first (the threshold a prune derives from them meets the victims
    at the insertion test), victims first (a later prune, with the impostors in the list, must keep them), shuffled (both,
    and across corpus splits), and the case no prune reaches (the rescore band alone)."""
    F = A.fixture(name)
    _check_exact(name, F, *_oracle(name))


@pytest.mark.parametrize("splits,window,variant", sorted(A.SPLIT_CASES))
def test_split_and_window_matrix(monkeypatch, splits, window, variant):
    """2, 4 and 8 corpus splits per query tile (65,536 / S queries, or the planner raises S), with and without windows:
    victims and impostors of a query land in different splits, so what a split adopts from its siblings -- at a prune, at a
    window boundary, in the rescore band's k-th score over two lists -- has to carry the slack (SPLIT_VARIANTS)."""
    monkeypatch.setenv("ANCE_FAST_SPLITS", str(splits))
    monkeypatch.setenv("ANCE_FAST_WINDOW_TILES", str(window))
    F = A.build(**A.SPLIT_CASES[(splits, window, variant)])
    assert A.plan_splits(F.n, len(F.q), F.k, splits) == splits
    _check_exact("adv_splits%d_window%d_%s" % (splits, window, variant), F, *_oracle((splits, window, variant), True))


@pytest.mark.parametrize("knobs", [{"ANCE_FAST_SHARE": "0", "ANCE_FAST_WINDOW_WAIT_US": "0"},
                                   {"ANCE_FAST_PRUNE_AT": "1", "ANCE_FAST_PRUNE_GROWTH": "105"},  # a prune at almost every tile
                                   {"ANCE_FAST_CENTER": "0"}, {"ANCE_FAST_DEDUP": "0"}],
                         ids=lambda kn: "-".join("%s=%s" % (k[10:], v) for k, v in kn.items()))
@pytest.mark.parametrize("name", A.KNOB_CASES)
def test_knobs_one_at_a_time(monkeypatch, knobs, name):
    for key, val in knobs.items():
        monkeypatch.setenv(key, val)
    F = A.fixture(name)
    _check_exact("adv_knob_%s_%s" % ("_".join(k[10:].lower() for k in knobs), name), F, *_oracle(name))


@pytest.mark.parametrize("name", ["unc_d128_n16384_k200_shuffled", "centred_d768_n8192_k200_imp_first",
                                  "qmean_d128_n16384_k200_vic_first", "unc_d2048_n4096_k50_shuffled"])
def test_audit_path_same_bits(name):
    """The same queries through the fp32 scan alone (search_device(..., exact_scan=True)) and through the filter."""
    F = A.fixture(name)
    idx = _check_exact(name + "_scan", F, *_oracle(name), exact_scan=True)
    _check_exact(name + "_fast", F, *_oracle(name), idx=idx)
