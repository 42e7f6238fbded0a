"""GPU: L2 search over the product-quantised lists, plain and residual (sonar_amd/csrc/ivf_pq_l2.hpp, sonar_amd/index.py;
DESIGN.md 3.30) against tests/ivf_pq_l2_ref.py.

The bias kernel is compared bit for bit with `prepare_rows(pq_decode(...))[1].neg()` (plain) and with the restatement (plain
and residual, both of its forms).  The plain search is, by contract, the flat L2 index over the decoded rows: compared bit for
bit, scores and ids, with an `IVFFlatL2Index` built over `pq_decode` of the codes under the same labels, on integer and on
real rows, and with the restatement on integer rows.  The residual search is compared bit for bit with the restatement on
integer data, where every term is exact and the distances are the int64 squared distances to c + r^; on real rows every
returned score lies within the bound tests/ivf_pq_l2_ref.py derives of its float64 value.  The data conditions these tests
rely on are asserted in tests/test_ivf_pq_l2_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_pq_l2_ref as Q
from tests import ivf_pq_ref as P
from tests import ivf_pq_residual_ref as PR
from tests import ivf_ref as R
from tests import l2_ref as L
from tests.test_gpu_ivf import _dev, _i32
from tests.test_gpu_ivf_regroup import _lists, _same_bits

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want_d, want_i):
    return np.array_equal(_bits(_np(got[0])), _bits(want_d)) and np.array_equal(_np(got[1]), want_i)


# ------------------------------------------------------------------------------------------------------ 1. the bias
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("d", [64, 192, 1024])
def test_bias_kernel_bit_for_bit(d, n):
    from sonar_amd import index
    from sonar_amd.xsim import prepare_rows

    k_lists = 3
    for dsub in (8, 16, 32, 64):
        rng = np.random.default_rng(d * 7 + n + dsub)
        m = d // dsub
        real_cb = (rng.standard_normal((m, 256, dsub)) * rng.uniform(0.01, 4.0, (m, 256, 1))).astype(np.float16)
        real_c = (rng.standard_normal((k_lists, d)) * 2.0).astype(np.float16)
        for cb, c in ((real_cb, real_c), (Q.scaled_integer_codebooks(rng, d, dsub), L.int_rows(rng, k_lists, d))):
            cb[:, 0] = 0  # codeword 0 of every sub-quantiser is zero: the all-zero code row decodes to a zero row
            codes = rng.integers(0, 256, (n, m)).astype(np.uint8)
            codes[n // 2] = 0
            labels = rng.integers(0, k_lists, n)
            labels[rng.random(n) < 0.2] = rng.choice(np.array([-1, k_lists, 2 ** 31 - 1]))  # no centroid
            cbd, cd, codesd = _dev(cb), _dev(c), _dev(codes)
            # plain: the half norms of the decoded rows, negated
            got = index.pq_l2_bias(codesd, cbd)
            want = prepare_rows(index.pq_decode(codesd, cbd))[1][:n].neg()
            assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (dsub, "prepare_rows")
            assert np.array_equal(_bits(_np(got)), _bits(Q.bias_plain(codes, cb))), (dsub, "plain")
            assert _bits(_np(got))[n // 2] == 0x80000000  # a zero row: -0, as prepare_rows(...)[1].neg() gives
            # residual, the stand-alone form over rows
            want_r = Q.bias_residual(codes, cb, labels, c)
            got_r = index.pq_l2_bias(codesd, cbd, _i32(labels), cd)
            assert np.array_equal(_bits(_np(got_r)), _bits(want_r)), (dsub, "residual")
            # the form over slots: the same values through the offsets, +0 in the pad and unused slots, whose codes
            # (garbage here) are not read
            off, sizes, ids = R.build(labels, k_lists)
            slot_ids = np.concatenate([ids, np.full(16, -1, dtype=np.int64)])  # unused slots behind offsets[K]
            slot_codes = np.where(slot_ids[:, None] >= 0, codes[np.maximum(slot_ids, 0)], 255).astype(np.uint8)
            sd, idd = _dev(slot_codes), _i32(slot_ids)
            got_s = index.pq_l2_bias(sd, cbd, None, cd, ids=idd, offsets=_i32(off))
            inside = (labels >= 0) & (labels < k_lists)  # (rows left out hold no slot)
            assert inside[slot_ids[slot_ids >= 0]].all()
            assert np.array_equal(_bits(_np(got_s)), _bits(Q.slot_bias(want_r, slot_ids))), (dsub, "residual slots")
            assert (_bits(_np(got_s))[slot_ids < 0] == 0).all()
            got_p = index.pq_l2_bias(sd, cbd, ids=idd)
            assert np.array_equal(_bits(_np(got_p)), _bits(Q.slot_bias(Q.bias_plain(codes, cb), slot_ids))), (dsub, "plain slots")


# ------------------------------------------------------------------------------------------------------ 2. the searches
@functools.lru_cache(maxsize=None)
def _case(n, nq, d, n_lists):
    """The integer case and what both classes make of it in numpy: codes, and the residual codes."""
    y, q, c, labels, cb = Q.int_case(n, nq, d, n_lists)
    codes, rcodes = P.encode(y, cb), PR.encode(y, labels, c, cb)
    for a in (y, q, c, labels, cb, codes, rcodes):
        a.setflags(write=False)
    return y, q, c, labels, cb, codes, rcodes


def _probe_tables(rng, nq, n_lists):
    probes = np.stack([rng.permutation(n_lists)[:4] for _ in range(nq)])
    probes[::3, 1] = -1          # entries that name no list
    probes[1::3, 2] = n_lists + 5
    probes[5] = [-1, 99, -7, n_lists]  # a query that probes nothing
    return probes


def _garbage_where_no_list(rng, coarse, probes, n_lists):
    coarse = np.array(coarse, dtype=np.float32)
    none = (probes < 0) | (probes >= n_lists)
    coarse[none] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], dtype=np.float32), int(none.sum()))
    return coarse


CASES = [(1500, 40, 64, 8), (1500, 300, 64, 8),     # 8 lists at nprobe 8: units of 64 pairs, and of 128 (2400 >= 2048)
         (1100, 40, 64, 12), (1100, 400, 64, 12), (1100, 70, 192, 12)]  # 12 lists: units of 128 from 3072 pairs on


@pytest.mark.parametrize("n,nq,d,n_lists", CASES)
def test_plain_search_is_the_flat_l2_index_over_the_decoded_rows(n, nq, d, n_lists):
    from sonar_amd import index
    from sonar_amd.xsim import prepare_rows

    y, q, c, labels, cb, codes, _ = _case(n, nq, d, n_lists)
    yd, qd, cd, cbd, ld = _dev(y), _dev(q), _dev(c), _dev(cb), _i32(labels)
    ix = index.IVFPQL2Index(cd, cbd).add(yd)  # labels by the quantiser: the Euclidean nearest centroid
    assert np.array_equal(np.bincount(labels, minlength=n_lists), _np(ix.list_sizes)) and ix.ntotal == n
    enc = index.pq_encode(prepare_rows(yd)[0], cbd, n)
    assert np.array_equal(_np(enc), codes)
    flat = index.IVFFlatL2Index(cd).add(index.pq_decode(enc, cbd), labels=ld)
    rng = np.random.default_rng(nq)
    own = _np(ix.probe(qd, 8))
    assert np.array_equal(own, L.topk(q, c, -L.half_norms(c), 8)[1])
    probes = _probe_tables(rng, nq, n_lists)
    for table in (own, probes):
        pd = _i32(table)
        for k in (1, 4, 8):
            got = ix.search(qd, k, probes=pd)
            want = flat.search(qd, k, probes=pd)
            assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), k
            want_d, want_i, _ = Q.search_plain(q, codes, cb, labels, n_lists, table, k)
            assert _same(got, want_d, want_i), k
    assert (want_i[5] == -1).all() and np.isposinf(want_d[5]).all()
    got = ix.search(qd, 8, 8)  # the index's own probe
    assert _same(got, *Q.search_plain(q, codes, cb, labels, n_lists, own, 8)[:2])
    # the distances are the exact squared distances to the decoded rows
    exact = Q.exact_sq_dist(q, Q.reconstruct(codes, cb))
    gd, gi = _np(got[0]), _np(got[1])
    assert (gi >= 0).all() and np.array_equal(gd.astype(np.int64), np.take_along_axis(exact, gi.astype(np.int64), axis=1))
    # the row mask
    visible = rng.random(n) < 0.4
    rows = ix.row_filter(mask=_dev(visible))
    got = ix.search(qd, 8, probes=_i32(probes), rows=rows)
    want_d, want_i, _ = Q.search_plain(q, codes, cb, labels, n_lists, probes, 8, visible)
    assert _same(got, want_d, want_i) and visible[want_i[want_i >= 0]].all() and (want_i == -1).any()
    want = flat.search(qd, 8, probes=_i32(probes), rows=flat.row_filter(mask=_dev(visible)))
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


@pytest.mark.parametrize("n,nq,d,n_lists", [(1500, 300, 64, 8), (1100, 70, 192, 12)])
def test_plain_search_on_real_rows_is_the_flat_l2_index_over_the_decoded_rows(n, nq, d, n_lists):
    from sonar_amd import index
    from sonar_amd.xsim import prepare_rows

    rng = np.random.default_rng(n + nq)
    y = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float16)
    q = (rng.standard_normal((nq, d)) * rng.uniform(0.5, 2.0, (nq, 1))).astype(np.float16)
    c, cb = y[:n_lists].copy(), P.random_codebooks(rng, d, 16, scale=8.0)
    yd, qd, cd, cbd = _dev(y), _dev(q), _dev(c), _dev(cb)
    ix = index.IVFPQL2Index(cd, cbd).add(yd)
    labels = ix.probe(yd, 1)[:, 0].contiguous()
    flat = index.IVFFlatL2Index(cd).add(index.pq_decode(index.pq_encode(prepare_rows(yd)[0], cbd, n), cbd), labels=labels)
    assert torch.equal(ix.list_sizes, flat.list_sizes)
    for k, nprobe in ((1, 1), (4, 3), (8, 8)):
        got, want = ix.search(qd, k, nprobe), flat.search(qd, k, nprobe)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (k, nprobe)
    assert (got[1] >= 0).all() and (got[0][:, 1:] >= got[0][:, :-1]).all()


@pytest.mark.parametrize("cls_name", ["IVFPQL2Index", "IVFPQResidualL2Index"])
def test_lists_of_three_rows_and_given_labels(cls_name):
    from sonar_amd import index

    y, q, c, _, cb, _, _ = _case(1100, 40, 64, 12)
    y = y[:36]
    labels = (np.arange(36) % 12).astype(np.int32)  # three rows per list, whatever the centroids say
    ix = getattr(index, cls_name)(_dev(c), _dev(cb)).add(_dev(y), labels=_i32(labels))
    assert (ix.list_sizes == 3).all()
    probes = np.stack([np.roll(np.arange(12), i)[:8] for i in range(40)])
    for table in (probes, probes[:, :2]):  # 24 candidates; 6 candidates: two fill entries
        got = ix.search(_dev(q), 8, probes=_i32(table))
        if cls_name == "IVFPQL2Index":
            want = Q.search_plain(q, P.encode(y, cb), cb, labels, 12, table, 8)
        else:
            want = Q.search_residual(q, PR.encode(y, labels, c, cb), cb, labels, c, table, None, 8)
        assert _same(got, want[0], want[1])
    assert (want[1][:, 6:] == -1).all() and np.isposinf(want[0][:, 6:]).all()


@pytest.mark.parametrize("n,nq,d,n_lists", CASES)
def test_residual_search_equals_the_restatement(n, nq, d, n_lists):
    from sonar_amd import index

    y, q, c, labels, cb, _, rcodes = _case(n, nq, d, n_lists)
    yd, qd, cd, cbd = _dev(y), _dev(q), _dev(c), _dev(cb)
    ix = index.IVFPQResidualL2Index(cd, cbd).add(yd)
    assert np.array_equal(np.bincount(labels, minlength=n_lists), _np(ix.list_sizes))
    rng = np.random.default_rng(nq + 1)
    own = _np(ix.probe(qd, 8))
    probes = _probe_tables(rng, nq, n_lists)
    exact = Q.exact_sq_dist(q, Q.reconstruct(rcodes, cb, labels, c))
    for table in (own, probes):
        pd = _i32(table)
        coarse = _garbage_where_no_list(rng, Q.coarse(q, c, table), table, n_lists)
        for k in (1, 4, 8):
            want_d, want_i, _ = Q.search_residual(q, rcodes, cb, labels, c, table, None, k)
            assert _same(ix.search(qd, k, probes=pd, coarse=_dev(coarse)), want_d, want_i), (k, "coarse given")
            assert _same(ix.search(qd, k, probes=pd), want_d, want_i), (k, "coarse by the index")
            have = want_i >= 0  # the distances are the exact integer squared distances to c + r^
            assert np.array_equal(want_d[have].astype(np.int64), np.take_along_axis(exact, np.maximum(want_i, 0), axis=1)[have])
    assert (want_i[5] == -1).all() and np.isposinf(want_d[5]).all()
    got = ix.search(qd, 8, 8)  # the index's own probe and its coarse terms
    assert _same(got, *Q.search_residual(q, rcodes, cb, labels, c, own, None, 8)[:2])
    assert np.array_equal(np.sort(exact, axis=1)[:, :8], _np(ix.search(qd, 8, min(8, n_lists))[0]).astype(np.int64)) or n_lists > 8
    visible = rng.random(n) < 0.4
    got = ix.search(qd, 8, probes=_i32(probes), rows=ix.row_filter(mask=_dev(visible)))
    want_d, want_i, _ = Q.search_residual(q, rcodes, cb, labels, c, probes, None, 8, visible)
    assert _same(got, want_d, want_i) and visible[want_i[want_i >= 0]].all()


@pytest.mark.parametrize("n,nq,d,n_lists,dsub", [(1500, 300, 64, 8, 8), (1100, 70, 192, 12, 32)])
def test_residual_scores_on_real_rows_within_the_bound_of_float64(n, nq, d, n_lists, dsub):
    from sonar_amd import index
    from sonar_amd.xsim import prepare_rows, topk_bias_prepared

    rng = np.random.default_rng(n + nq + 2)
    y = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float16)
    q = (rng.standard_normal((nq, d)) * rng.uniform(0.5, 2.0, (nq, 1))).astype(np.float16)
    c, cb = y[:n_lists].copy(), P.random_codebooks(rng, d, dsub, scale=6.0)
    cd, cbd = _dev(c), _dev(cb)
    y16, _ = prepare_rows(_dev(y))
    q16, _ = prepare_rows(_dev(q))
    c16, ch = prepare_rows(cd)
    labels = topk_bias_prepared(y16, n, c16, n_lists, ch.neg(), 1)[1][:, 0].contiguous()
    codes_rows = index.pq_encode_residual(y16, labels, cd, cbd)
    codes, ids, off, _ = index.build_lists_pq_residual(y16, labels, cd, cbd)
    bias = index.pq_l2_bias(codes, cbd, None, cd, ids=ids, offsets=off)
    nprobe = min(8, n_lists)
    coarse, probes = topk_bias_prepared(q16, nq, c16, n_lists, ch.neg(), nprobe)
    score, idx = index.search_lists_pq_l2(q16, probes, codes, cbd, bias, ids, off, 8, coarse)
    torch.cuda.synchronize()
    s64, bound = Q.residual_score_bound(q, _np(codes_rows), cb, _np(labels), c)
    score, idx = _np(score).astype(np.float64), _np(idx).astype(np.int64)
    assert (idx >= 0).all()
    err = np.abs(score - np.take_along_axis(s64, idx, axis=1))
    lim = np.take_along_axis(bound, idx, axis=1)
    print("largest error / bound:", float((err / lim).max()), "largest bound:", float(lim.max()))
    assert (err <= lim).all()  # no row is excused
    if nprobe == n_lists:  # every list probed: the best score is within the bound of the best float64 score
        assert (s64.max(axis=1) - score[:, 0] <= bound.max(axis=1)).all()


# ------------------------------------------------------------------------------------------------------ 3. further checks
def _storage(ix):
    return ix._rows, ix._codebooks, ix._bias, ix._ids, ix._offsets


@pytest.mark.parametrize("cls_name", ["IVFPQL2Index", "IVFPQResidualL2Index"])
def test_a_pad_slot_with_a_winning_bias_never_enters_and_the_bits_do_not_depend_on_company(cls_name):
    from sonar_amd import index
    from sonar_amd.xsim import prepare_rows

    y, q, c, labels, cb, _, _ = _case(1100, 70, 192, 12)
    ix = getattr(index, cls_name)(_dev(c), _dev(cb)).add(_dev(y))
    qd = _dev(q)
    q16, _ = prepare_rows(qd)
    coarse, probes = ix._nearest_lists(q16, 70, 4)
    coarse = coarse if cls_name == "IVFPQResidualL2Index" else None
    codes, cbd, bias, ids, off = _storage(ix)
    a = index.search_lists_pq_l2(q16, probes, codes, cbd, bias, ids, off, 8, coarse)
    assert (ids < 0).any() and (bias[ids < 0] == 0).all()
    loud = torch.where(ids < 0, torch.full_like(bias, 1e30), bias)
    b = index.search_lists_pq_l2(q16, probes, codes, cbd, loud, ids, off, 8, coarse)
    assert _same_bits(a, b) and (a[1] >= 0).all()
    # two calls, and a subset of the queries
    full = ix.search(qd, 8, 4)
    assert _same_bits(full, ix.search(qd, 8, 4))
    pick = torch.tensor([0, 3, 17, 64, 69], device="cuda")
    part = ix.search(qd[pick].contiguous(), 8, 4)
    assert _same_bits(part, (full[0][pick], full[1][pick]))
    one = ix.search(qd[68:69].contiguous(), 8, 4)
    assert _same_bits(one, (full[0][68:69], full[1][68:69]))


@pytest.mark.parametrize("cls_name", ["IVFPQL2Index", "IVFPQResidualL2Index"])
def test_state_dict_round_trip_and_one_capture(cls_name):
    from sonar_amd import index

    y, q, c, labels, cb, codes, rcodes = _case(1100, 70, 192, 12)
    cls = getattr(index, cls_name)
    residual = cls_name == "IVFPQResidualL2Index"
    ix = cls(_dev(c), _dev(cb)).add(_dev(y))
    state = ix.state_dict()
    want_keys = {"centroids", "offsets", "sizes", "rows", "bias", "ids", "codebooks", "metric_l2"} | ({"by_residual"} if residual else set())
    assert set(state) == want_keys
    used = int(state["offsets"][12])
    assert state["rows"].shape == (used, 192 // 8) and state["rows"].dtype == torch.uint8 and state["bias"].shape == (used,)
    ids = _np(state["ids"])
    row_bias = Q.bias_residual(rcodes, cb, labels, c) if residual else Q.bias_plain(codes, cb)
    assert np.array_equal(_bits(_np(state["bias"])), _bits(Q.slot_bias(row_bias, ids)))
    assert np.array_equal(_np(state["rows"])[ids >= 0], (rcodes if residual else codes)[ids[ids >= 0]])
    qd = _dev(q)
    a = ix.search(qd, 8, 4)
    assert _same_bits(a, cls.from_state_dict(state).search(qd, 8, 4))
    other = cls(_dev(c), _dev(cb))
    other.load_state_dict(state)
    assert _same_bits(a, other.search(qd, 8, 4))
    for wrong in ("IVFPQIndex", "IVFPQResidualIndex", "IVFFlatIndex", "IVFFlatL2Index",
                  "IVFPQL2Index" if residual else "IVFPQResidualL2Index"):
        with pytest.raises(ValueError):
            getattr(index, wrong).from_state_dict(state)
    # one capture of search with given probes
    probes = ix.probe(qd, 4)
    eager = ix.search(qd, 8, probes=probes)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ix.search(qd, 8, probes=probes)  # warm-up: the one-time attribute calls
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ix.search(qd, 8, probes=probes)
    out[0].fill_(0), out[1].fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, eager) and torch.equal(eager[1], a[1])


def test_refusals_launch_nothing():
    from sonar_amd import _lib, index
    from sonar_amd.xsim import prepare_rows

    lib = _lib.load()
    y, q, c, labels, cb, _, _ = _case(1100, 40, 64, 12)
    ix = index.IVFPQResidualL2Index(_dev(c), _dev(cb)).add(_dev(y))
    codes, cbd, bias, ids, off = _storage(ix)
    q16, _ = prepare_rows(_dev(q))
    coarse, probes = ix._nearest_lists(q16, 40, 4)
    nq, d, nprobe, K, k, guard, SENT = 40, 64, 4, 12, 4, 256, -77
    need = int(lib.smi_l2_pq_search_ws_bytes(nq, K, nprobe, k, d, 8))
    big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = big[guard:guard + need]
    idx = torch.full((nq, k), SENT, dtype=torch.int32, device="cuda")
    score = torch.full((nq, k), float(SENT), dtype=torch.float32, device="cuda")
    out = torch.full((codes.shape[0],), float(SENT), dtype=torch.float32, device="cuda")
    st = _lib.current_stream_ptr()
    p = lambda t: t.data_ptr()  # noqa: E731

    def S(dsub=8, cb_=p(cbd), bias_=p(bias), k_=k, ws_bytes=need, d_=d):
        return lib.smi_l2_pq_search(p(q16), nq, d_, p(probes), nprobe, p(codes), dsub, cb_, bias_, p(ids), p(off), K, k_, p(idx), p(score),
                                    p(ws), ws_bytes, st)

    def Rs(coarse_=p(coarse), bias_=p(bias), ws_bytes=need):
        return lib.smi_l2_pq_search_residual(p(q16), nq, d, p(probes), coarse_, nprobe, p(codes), 8, p(cbd), bias_, p(ids), p(off), K, k,
                                             p(idx), p(score), p(ws), ws_bytes, st)

    def B(cent=None, labels_=None, off_=None, ids_=None, dsub=8, cb_=p(cbd)):
        return lib.smi_l2_pq_bias(p(codes), codes.shape[0], d, dsub, cb_, ids_, off_, labels_, cent, K if cent else 0, p(out), st)

    refused = [S(dsub=12), S(cb_=None), S(cb_=p(cbd) + 8), S(bias_=None), S(bias_=p(bias) + 4), S(k_=9), S(ws_bytes=need - 1), S(d_=96),
               Rs(coarse_=None), Rs(coarse_=p(coarse) + 2), Rs(bias_=p(bias) + 8), Rs(ws_bytes=need - 1),
               B(dsub=12), B(cb_=None), B(labels_=p(ids)), B(cent=p(ix._c16)), B(cent=p(ix._c16), labels_=p(ids), off_=p(off), ids_=p(ids)),
               B(cent=p(ix._c16), off_=p(off))]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert (idx == SENT).all() and (score == SENT).all() and (out == SENT).all() and (big == 0xA5).all()
    _lib.check(Rs())
    torch.cuda.synchronize()
    want = index.search_lists_pq_l2(q16, probes, codes, cbd, bias, ids, off, k, coarse)
    assert _same_bits((score, idx), want)
    assert (big[:guard] == 0xA5).all() and (big[guard + need:] == 0xA5).all()


def _make(cls_name):
    from sonar_amd import index

    _, _, c, _, cb, _, _ = _case(1100, 70, 192, 12)
    return lambda: getattr(index, cls_name)(_dev(c), _dev(cb))


def _assert_same_index(got, want, q, what):
    assert torch.equal(got.list_sizes, want.list_sizes) and torch.equal(got.list_offsets, want.list_offsets), what
    assert _lists(got) == _lists(want), what  # per list: ids, code bytes and bias bits
    for k, nprobe in ((1, 1), (8, 5)):
        assert _same_bits(got.search(q, k=k, nprobe=nprobe), want.search(q, k=k, nprobe=nprobe)), (what, k, nprobe)


@pytest.mark.parametrize("cls_name", ["IVFPQL2Index", "IVFPQResidualL2Index"])
def test_extend_remove_and_merge_equal_the_one_shot_add(cls_name):
    make = _make(cls_name)
    y, q, _, _, _, _, _ = _case(1100, 70, 192, 12)
    x, qd = _dev(y), _dev(q)
    n1 = 700
    want = make().add(x)
    got = make().add(x[:n1])
    assert got.extend(x[n1:]) is got and got._generation == 1
    _assert_same_index(got, want, qd, "extend")
    _assert_same_index(make().add(x[:100]).extend(x[100:n1]).extend(x[n1:]), want, qd, "extend in three chunks")
    a, b = make().add(x[:n1]), make().add(x[n1:])
    assert a.merge_from(b) is a
    _assert_same_index(a, want, qd, "merge_from")
    drop = torch.from_numpy(np.random.default_rng(3).random(1100) < 0.3).cuda()
    lab = want.probe(x, 1)[:, 0]
    without = make().add(x, torch.where(drop, torch.full_like(lab, -1), lab).contiguous())
    _assert_same_index(make().add(x).remove(mask=drop), without, qd, "remove by mask")
    _assert_same_index(make().add(x).remove(ids=torch.nonzero(drop)[:, 0]), without, qd, "remove by ids")
    with pytest.raises(TypeError, match="merge_from"):
        a.merge_from(_make("IVFPQL2Index" if cls_name == "IVFPQResidualL2Index" else "IVFPQResidualL2Index")().add(x[:50]))


@pytest.mark.parametrize("cls_name", ["IVFPQL2Index", "IVFPQResidualL2Index"])
def test_train_add_search_refine_on_planted_rows(cls_name):
    from sonar_amd import index
    from sonar_amd.xsim import prepare_rows

    px, py, truth = L.planted()
    xd, yd = _dev(px), _dev(py)
    ix = getattr(index, cls_name).train(yd, 6, dsub=8, n_iter=3, pq_iter=3).add(yd)
    assert ix.n_lists == 6 and ix.dsub == 8 and ix.ntotal == len(py)
    raw = ix.search(xd, 8, 6)
    assert (raw[1] >= 0).all() and (raw[0][:, 1:] >= raw[0][:, :-1]).all()
    corpus = prepare_rows(yd)
    dist, idx = ix.search(xd, 8, 6, refine=corpus)
    assert np.array_equal(_np(idx)[:, 0], truth[:, 0])  # the planted neighbour is first for every row
    assert np.array_equal(np.sort(_np(idx), axis=1), np.sort(_np(raw[1]), axis=1))  # the same candidates, re-ordered
    # the refined distances are those to the fp16 rows, within the bound of the flat scores
    exact = ((px.astype(np.float64)[:, None, :] - py.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    tol = 4 * L.planted_gap(px, py, truth)[1] + 2.0 ** -21 * float(L.half_norms(px).max())
    assert np.abs(_np(dist).astype(np.float64) - np.take_along_axis(exact, _np(idx).astype(np.int64), axis=1)).max() <= tol
    assert (dist[:, 1:] >= dist[:, :-1]).all()


@pytest.mark.parametrize("cls_name", ["IVFPQL2Index", "IVFPQResidualL2Index"])
def test_behind_a_signed_permutation_it_is_the_bare_index_over_the_permuted_rows(cls_name):
    from sonar_amd import index
    from sonar_amd.transforms import LinearTransform

    y, q, c, labels, cb, _, _ = _case(1100, 40, 128, 12)  # (a transform's d_out is a multiple of 128)
    rng = np.random.default_rng(11)
    perm, sign = rng.permutation(128), rng.choice(np.array([-1.0, 1.0]), 128)
    w = np.zeros((128, 128))
    w[np.arange(128), perm] = sign  # out[j] = sign[j] * x[perm[j]]
    t = LinearTransform(_dev(w))
    cls = getattr(index, cls_name)
    wrapped = index.PreTransformIndex(t, cls(_dev(c), _dev(cb))).add(_dev(y))
    half0 = np.float16(0.0)  # (-0 + 0 = +0: the transform's sums start from +0)
    yp, qp = y[:, perm] * sign.astype(np.float16) + half0, q[:, perm] * sign.astype(np.float16) + half0
    bare = cls(_dev(c), _dev(cb)).add(_dev(np.ascontiguousarray(yp)))
    assert _lists(wrapped.index) == _lists(bare)
    qd, qpd = _dev(q), _dev(np.ascontiguousarray(qp))
    for k, nprobe in ((1, 1), (8, 6)):
        assert _same_bits(wrapped.search(qd, k, nprobe), bare.search(qpd, k, nprobe)), (k, nprobe)
    with pytest.raises(TypeError, match=r"index\.search\(transform\.apply\(q\), refine="):
        wrapped.search(qd, 8, 6, refine=_dev(y))
