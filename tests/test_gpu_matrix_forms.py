"""Non-canonical matrix input on every engine (contract of include/rsqp_hip.h): a CSC array or a triplet list describes the SUM of its
entries, whatever the order of the rows within a column. Each case solves an input with rows out of order (`shuffle`), split
entries (`split`), a full entry count whose canonical form has one entry less (`fullcount`) or a cancelling pair (`cancel`), and
checks it against the same engine on the canonical input (bit for bit) and against the CPU oracle on the canonical form. Every
case asserts the kernel or path it means to reach, so that a change of dispatch cannot move it quietly."""
import numpy as np
import pytest

from conftest import oracle_cold
from restartsqp_amd import problems
from restartsqp_amd.batch_problems import handler_shaped_qp
from restartsqp_amd.qpdump import csc_to_dense, dense_to_csc
from test_gpu_large_engine import _diag_h_qp
from test_gpu_parity import assert_same_solution
from test_matrix_forms import canonical_qp, cancel, fullcount, integer_dense, shuffle, split, with_matrices

pytestmark = pytest.mark.gpu


def _vectors(s, q):
    for w, v in zip(range(5), (q.g, q.lb, q.ub, q.lbA, q.ubA)):
        s.set_vector(w, v)


def _state(s, n):
    wb, wc = s.working_set_raw()
    return (n, s.status, s.x.copy(), s.y.copy(), wb.copy(), wc.copy(), s.objective)


def _bit_same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[6] == b[6], (a[0], b[0], a[1], b[1], a[6], b[6])
    for u, v in zip(a[2:6], b[2:6]):
        assert np.array_equal(u, v)


def _transform(rng, kind, nrow, ncol, jc, ir, val):
    if kind == "shuffle":
        return shuffle(rng, jc, ir, val)
    if kind == "split":
        return split(rng, jc, ir, val)
    if kind == "cancel":
        return cancel(rng, nrow, jc, ir, val)
    raise ValueError(kind)


# --------------------------------------------------------------------------
# products: integer data, so every sum is exact and must bit-equal numpy on the summed dense matrix
# --------------------------------------------------------------------------
def _check_products(s, A, H, rng):
    p = rng.integers(-8, 9, size=A.shape[1]).astype(float); r = rng.integers(-8, 9, size=A.shape[0]).astype(float)
    assert np.array_equal(s.A_times(p), A @ p)
    assert np.array_equal(s.A_transposed_times(r), A.T @ r)
    assert np.array_equal(s.H_times(p), H @ p)


def _triplet_dense(n, m, irow, jcol, val, sym=False):
    D = np.zeros((n, m))
    np.add.at(D, (np.asarray(irow) - 1, np.asarray(jcol) - 1), val)
    if sym:
        off = np.asarray(irow) != np.asarray(jcol)
        np.add.at(D, (np.asarray(jcol)[off] - 1, np.asarray(irow)[off] - 1), np.asarray(val)[off])
    return D


@pytest.mark.parametrize("handle", ["arena0", "arena1", "hbm_dense", "hbm_sparse"])
def test_products_after_upload_and_refresh(capi, monkeypatch, handle):
    rng = np.random.default_rng(11)
    nV, nC = (6, 5) if handle.startswith("arena") else (120, 100)
    if handle.startswith("arena"):
        monkeypatch.setenv("RSQP_ARENA_MAPPED", handle[-1])
    dens = 0.3 if handle == "hbm_sparse" else 1.0
    for kind in ("shuffle", "split", "fullcount", "cancel"):
        if kind == "fullcount" and dens < 1.0:
            continue
        Ad = integer_dense(rng, nC, nV, min(dens, 0.6) if kind == "cancel" else dens)    # (cancel: a position without entry)
        S = integer_dense(rng, nV, nV, 0.5); Hd = S + S.T + np.diag(np.full(nV, 40.0))
        if kind == "fullcount":
            Aform, Ad = fullcount(rng, Ad)
        else:
            Aform = _transform(rng, kind, nC, nV, *dense_to_csc(Ad))
        Hform = shuffle(rng, *dense_to_csc(Hd)) if kind == "shuffle" else split(rng, *dense_to_csc(Hd))
        s = capi.Solver(nV, nC)
        assert s.engine == (1 if handle.startswith("arena") else 2)
        s.set_A_csc(*Aform); s.set_H_csc(*Hform)
        _check_products(s, Ad, Hd, rng)
        jc, ir, val, _ = s.get_A_csc()                 # the caller's layout, as given
        assert np.array_equal(jc, Aform[0]) and np.array_equal(ir, Aform[1]) and np.array_equal(val, Aform[2])
        A2 = rng.integers(-8, 9, size=len(Aform[2])).astype(float)      # same-pattern CSC refresh in the caller's layout
        s.set_A_csc(Aform[0], Aform[1], A2); s.set_H_csc(Hform[0], Hform[1], 2.0 * Hform[2])
        _check_products(s, csc_to_dense(nC, nV, Aform[0], Aform[1], A2), 2.0 * Hd, rng)
        assert np.array_equal(s.get_A_csc()[2], A2) and np.array_equal(s.get_H_csc()[2], 2.0 * Hform[2])
        s.close()
    # triplets: repeated positions kept in the CSC (SpHbMat), summed by the products, refreshed through order_
    Ad = integer_dense(rng, nC, nV, dens)
    rr, cc = np.nonzero(Ad)
    dup = rng.random(len(rr)) < 0.3
    irow = np.concatenate([rr, rr[dup]]) + 1; jcol = np.concatenate([cc, cc[dup]]) + 1
    tv = np.concatenate([Ad[rr, cc], rng.integers(-8, 9, size=dup.sum()).astype(float)])
    Hu = np.triu(integer_dense(rng, nV, nV, 0.3), 1) + 20.0 * np.eye(nV)
    hr, hc = np.nonzero(Hu)
    hi = np.concatenate([hr, [0, 0]]) + 1; hj = np.concatenate([hc, [0, 1]]) + 1     # a repeated diagonal and off-diagonal entry
    hv = np.concatenate([Hu[hr, hc], [3.0, 2.0]])
    s = capi.Solver(nV, nC)
    s.set_A_triplet(irow, jcol, tv); s.set_H_triplet(hi, hj, hv, True)
    _check_products(s, _triplet_dense(nC, nV, irow, jcol, tv), _triplet_dense(nV, nV, hi, hj, hv, True), rng)
    tv2 = rng.integers(-8, 9, size=len(tv)).astype(float); hv2 = hv + 1.0
    s.set_A_triplet(irow, jcol, tv2); s.set_H_triplet(hi, hj, hv2, True)
    _check_products(s, _triplet_dense(nC, nV, irow, jcol, tv2), _triplet_dense(nV, nV, hi, hj, hv2, True), rng)
    s.close()


# --------------------------------------------------------------------------
# single-QP handles: cold, hot on new vectors, hot on new matrices (CSC refresh in the caller's layout)
# --------------------------------------------------------------------------
def _handle_seq(capi, q, q2, A, H, A2, H2, how, engine=None):
    s = capi.Solver(q.nV, q.nC)
    if engine:
        s.set_engine(engine)
    s.set_options(20000, 100)
    s.set_A_csc(*A); s.set_H_csc(*H)
    _vectors(s, q)
    go = (lambda m: s.optimize_qp()) if how == "optimize" else (lambda m: s.solve(m, 20000))
    out = [_state(s, go(capi.MODE_COLD))]
    paths = [s.large_path()]
    cert = s.test_optimality()
    _vectors(s, q2)
    out.append(_state(s, go(capi.MODE_HOT_VECTORS)))
    s.set_A_csc(A[0], A[1], A2); s.set_H_csc(H[0], H[1], H2)
    out.append(_state(s, go(capi.MODE_HOT_MATRICES)))
    paths.append(s.large_path())
    s.close()
    return out, paths, cert


def _against_oracle(oracle, q, q2, kA2, kH2, out):
    qp, rc, n = oracle_cold(oracle, canonical_qp(q), 20000)
    _oracle_same(out[0], qp, n)
    rc, n = qp.hotstart(q2.g, q2.lb, q2.ub, q2.lbA, q2.ubA, 20000)
    _oracle_same(out[1], qp, n)
    qp.set_A_csc(*kA2); qp.set_H_csc(*kH2)
    rc, n = qp.hotstart_matrices(q2.g, q2.lb, q2.ub, q2.lbA, q2.ubA, 20000)
    _oracle_same(out[2], qp, n)


def _oracle_same(st, qp, n_or):
    assert_same_solution(qp, dict(status=st[1], x=st[2], y=st[3], ws_b=st[4], ws_c=st[5], nWSR=st[0]), n_or)


def _forms_and_check(capi, oracle, rng, q, kinds, how="solve", engine=None, want_path=None, Aform=None):
    """the same call sequence on the canonical input and on each non-canonical form; bit-identical results, and the oracle"""
    q2 = problems.perturb(rng, q, 0.05)
    A2c = q.A_val * (1.0 + 0.01 * rng.normal(size=len(q.A_val))); H2c = q.H_val * 1.05
    base, paths, cert0 = _handle_seq(capi, q, q2, (q.A_jc, q.A_ir, q.A_val), (q.H_jc, q.H_ir, q.H_val), A2c, H2c, how, engine)
    again, _, _ = _handle_seq(capi, q, q2, (q.A_jc, q.A_ir, q.A_val), (q.H_jc, q.H_ir, q.H_val), A2c, H2c, how, engine)
    for a, b in zip(base, again):
        _bit_same(a, b)                                # (the engine is reproducible: the bar below is exact)
    if want_path is not None:
        assert paths == [want_path, want_path], paths
    for kind in kinds:
        if kind == "split_A" or kind in ("shuffle", "split"):
            k = "split" if kind == "split_A" else kind
            A = _transform(rng, k, q.nC, q.nV, q.A_jc, q.A_ir, q.A_val)
        elif kind == "fullcount":
            A = Aform
        else:
            A = (q.A_jc, q.A_ir, q.A_val)
        H = _transform(rng, kind, q.nV, q.nV, q.H_jc, q.H_ir, q.H_val) if kind in ("shuffle", "split") else (q.H_jc, q.H_ir, q.H_val)
        # refreshed values in each layout that describe the canonical refresh exactly (halves of a split value, permuted order)
        A2 = _relayout(A, q.A_jc, q.A_ir, A2c, q.nC); H2 = _relayout(H, q.H_jc, q.H_ir, H2c, q.nV)
        out, p2, cert = _handle_seq(capi, q, q2, A, H, A2, H2, how, engine)
        assert p2 == paths, (kind, p2, paths)
        for a, b in zip(base, out):
            _bit_same(a, b)
        assert cert[0] == cert0[0] and cert[1].KKT_error == cert0[1].KKT_error
        assert np.array_equal(cert[2], cert0[2]) and np.array_equal(cert[3], cert0[3])
    if how == "optimize":      # (optimizeQP picks its own call shapes: the oracle's bar on the first, cold, QP)
        qp, rc, n = oracle_cold(oracle, q, 20000)
        _oracle_same(base[0], qp, n)
    else:
        _against_oracle(oracle, q, q2, (q.A_jc, q.A_ir, A2c), (q.H_jc, q.H_ir, H2c), base)
    return base


def _relayout(form, jc0, ir0, v0, nrow):
    """values for the layout `form` (a shuffle / split / fullcount of the canonical (jc0, ir0)) whose canonical sum is v0 exactly:
    every entry of a position gets the position's value divided by the number of its entries (1 or 2: exact)"""
    jc, ir = form[0], form[1]
    ncol = len(jc) - 1
    col = np.repeat(np.arange(ncol), np.diff(jc))
    key = col.astype(np.int64) * nrow + ir
    col0 = np.repeat(np.arange(ncol), np.diff(jc0))
    key0 = col0.astype(np.int64) * nrow + np.asarray(ir0)
    pos = {int(k): i for i, k in enumerate(key0)}
    cnt = {}
    for k in key.tolist():
        cnt[k] = cnt.get(k, 0) + 1
    return np.array([v0[pos[k]] / cnt[k] if k in pos else 0.0 for k in key.tolist()])


def test_tableau_handle_up_to_8x8(capi, oracle):
    """hs071-scale handles (the register-resident tableau kernel): CSC shuffle / split, the split of a single H[r,c] slot (h_sym),
    and triplets with repeated entries -- a symmetric H list with a repeated diagonal and off-diagonal entry"""
    rng = np.random.default_rng(21)
    q = problems.hs071_first_qp()
    _forms_and_check(capi, oracle, rng, q, ("shuffle", "split", "split_A"), how="optimize")
    # one split H[r, c] slot (r != c): before the fold, the tableau's symmetry test saw half a value on one side
    q6 = problems.random_qp(rng, 6, 4, 0.7)
    off = [k for c in range(6) for k in range(q6.H_jc[c], q6.H_jc[c + 1]) if q6.H_ir[k] != c][0]
    H1 = split(rng, q6.H_jc, q6.H_ir, q6.H_val, only=[off])
    q62 = problems.perturb(np.random.default_rng(5), q6, 0.05)
    b0, _, _ = _handle_seq(capi, q6, q62, (q6.A_jc, q6.A_ir, q6.A_val), (q6.H_jc, q6.H_ir, q6.H_val), q6.A_val, q6.H_val, "optimize")
    b1, _, _ = _handle_seq(capi, q6, q62, (q6.A_jc, q6.A_ir, q6.A_val), H1, q6.A_val,
                           _relayout(H1, q6.H_jc, q6.H_ir, q6.H_val, 6), "optimize")
    for a, b in zip(b0, b1):
        _bit_same(a, b)
    # triplets: A with repeated positions, H as a symmetric triangle with a repeated diagonal and off-diagonal entry
    Ad = q.dense_A(); Hd = q.dense_H()
    rr, cc = np.nonzero(Ad)
    irow = np.concatenate([rr, rr[:2]]) + 1; jcol = np.concatenate([cc, cc[:2]]) + 1
    tv = np.concatenate([Ad[rr, cc], [0.0, 0.0]]); tv[:2] *= 0.5; tv[-2:] = tv[:2]
    hr, hc = np.nonzero(np.triu(Hd))
    d0 = int(np.nonzero(hr == hc)[0][0]); o0 = int(np.nonzero(hr != hc)[0][0])
    hi = np.concatenate([hr, [hr[d0], hr[o0]]]) + 1; hj = np.concatenate([hc, [hc[d0], hc[o0]]]) + 1
    hv = np.concatenate([Hd[hr, hc], [0.0, 0.0]]); hv[[d0, o0]] *= 0.5; hv[-2:] = hv[[d0, o0]]
    res = []
    for trip in (False, True):
        s = capi.Solver(q.nV, q.nC)
        if trip:
            s.set_A_triplet(irow, jcol, tv); s.set_H_triplet(hi, hj, hv, True)
            assert s.get_A_csc()[2].size == len(tv)
        else:
            s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        _vectors(s, q)
        st = [_state(s, s.optimize_qp())]
        q2 = problems.perturb(np.random.default_rng(8), q, 0.05)
        _vectors(s, q2)
        st.append(_state(s, s.optimize_qp()))
        if trip:
            s.set_A_triplet(irow, jcol, 1.5 * tv); s.set_H_triplet(hi, hj, 1.5 * hv, True)
        else:
            s.set_A_csc(q.A_jc, q.A_ir, 1.5 * q.A_val); s.set_H_csc(q.H_jc, q.H_ir, 1.5 * q.H_val)
        st.append(_state(s, s.optimize_qp()))
        res.append(st)
        s.close()
    for a, b in zip(*res):
        _bit_same(a, b)


@pytest.mark.parametrize("engine", ["0", "1"])
def test_lds_mid_size_handle(capi, oracle, monkeypatch, engine):
    monkeypatch.setenv("RSQP_SMALL_ENGINE", engine)
    rng = np.random.default_rng(31)
    q = problems.random_qp(rng, 30, 20, 0.4)
    _forms_and_check(capi, oracle, rng, q, ("shuffle", "split"), how="solve", engine=1)


@pytest.mark.parametrize("path", [0, 1, 2, 4])
def test_hbm_engine_handle(capi, oracle, path):
    rng = np.random.default_rng(41 + path)
    Aform = None
    if path == 0:
        q = handler_shaped_qp(rng, 60, 40, definite=False)
    elif path == 1:
        q = _diag_h_qp(rng, 130, 60, 0.3)
    elif path == 2:
        q = problems.banded_qp(rng, 150, 60, 0.3)
    else:
        q = problems.random_qp(rng, 120, 30, 1.0)     # dense A: the full-count form as well
        Ad = q.dense_A()
        Aform, Ad = fullcount(rng, Ad)
        q = with_matrices(q, A=dense_to_csc(Ad))
    assert q.nV >= 120
    kinds = ("shuffle", "split") + (("fullcount",) if Aform is not None else ())
    _forms_and_check(capi, oracle, rng, q, kinds, how="solve", engine=2, want_path=path, Aform=Aform)


# --------------------------------------------------------------------------
# batches: cold, hot on new vectors, hot on new matrices (rsqp_batch_set_matrix_values in the caller's layout)
# --------------------------------------------------------------------------
def _batch_seq(capi, probs, probs2, vals2):
    b = capi.Batch(probs, device=0)
    b.solve(capi.MODE_COLD, 20000)
    kern = [b.last_kernel()]
    out = [b.results()]
    cert = b.test_optimality()
    b.set_vectors_from(probs2)
    b.solve(capi.MODE_HOT_VECTORS, 20000)
    out.append(b.results())
    b.set_matrix_values(*vals2)
    b.solve(capi.MODE_HOT_MATRICES, 20000)
    out.append(b.results())
    kern.append(b.last_kernel())
    b.close()
    return out, kern, cert


def _res_same(r1, r2):
    for a, b in zip(r1, r2):
        assert a["status"] == b["status"] and a["nWSR"] == b["nWSR"] and a["obj"] == b["obj"]
        for k in ("x", "y", "ws_b", "ws_c"):
            assert np.array_equal(a[k], b[k]), k


def _batch_check(capi, oracle, rng, probs, forms, want_kernel, hot=True):
    probs2 = [problems.perturb(rng, q, 0.02) for q in probs]
    A2 = [q.A_val * (1.0 + 0.01 * rng.normal(size=len(q.A_val))) for q in probs]
    H2 = [q.H_val * 1.05 for q in probs]
    cat = lambda xs: np.concatenate(xs + [np.zeros(0)])
    base, kern, cert0 = _batch_seq(capi, probs, probs2, (cat(A2), cat(H2)))
    assert kern[0] == want_kernel, kern        # (the lane kernel takes cold starts only: its hot starts run on the 8-lane one)
    again, _, _ = _batch_seq(capi, probs, probs2, (cat(A2), cat(H2)))
    for a, b in zip(base, again):
        _res_same(a, b)
    for form in forms:
        nf = [form(q) for q in probs]
        fA2 = [_relayout((f.A_jc, f.A_ir), q.A_jc, q.A_ir, a2, q.nC) for f, q, a2 in zip(nf, probs, A2)]
        fH2 = [_relayout((f.H_jc, f.H_ir), q.H_jc, q.H_ir, h2, q.nV) for f, q, h2 in zip(nf, probs, H2)]
        nf2 = [with_matrices(p2, (f.A_jc, f.A_ir, f.A_val), (f.H_jc, f.H_ir, f.H_val)) for f, p2 in zip(nf, probs2)]
        out, k2, cert = _batch_seq(capi, nf, nf2, (cat(fA2), cat(fH2)))
        assert k2 == kern
        if getattr(form, "exact", True):
            for a, b in zip(base, out):
                _res_same(a, b)
            assert np.array_equal(cert[0], cert0[0]) and cert[1] == cert0[1]
        else:          # a cancelling pair stores a 0.0 the canonical input does not have: the oracle's bar
            for f, r in zip(nf, out[0]):
                qp, rc, n = oracle_cold(oracle, canonical_qp(f), 20000)
                assert_same_solution(qp, r, n)
            assert np.all(cert[0] == 1)
        assert np.all(cert0[0] == 1)
    for q, r in zip(probs, base[0]):
        qp, rc, n = oracle_cold(oracle, q, 20000)
        assert_same_solution(qp, r, n)


def _form(kind, seed):
    rng = np.random.default_rng(seed)

    def f(q):
        A = _transform(rng, kind, q.nC, q.nV, q.A_jc, q.A_ir, q.A_val)
        H = _transform(rng, "split" if kind == "cancel" else kind, q.nV, q.nV, q.H_jc, q.H_ir, q.H_val)     # (H: dense)
        return with_matrices(q, A, H)
    f.exact = kind != "cancel"
    return f


def _same_split(q0):
    """one split pattern for every member (the lane kernel's one-pattern batch): the same slots of A and H split in each"""
    ka = [int(q0.A_jc[1])]; kh = [int(q0.H_jc[0])]

    def f(q):
        return with_matrices(q, split(None, q.A_jc, q.A_ir, q.A_val, only=ka), split(None, q.H_jc, q.H_ir, q.H_val, only=kh))
    return f


@pytest.mark.parametrize("lane", ["1", "0"])
def test_batch_hs071_scale(capi, oracle, monkeypatch, lane):
    monkeypatch.setenv("RSQP_LANE", lane)
    rng = np.random.default_rng(51)
    probs = problems.hs071_scale_batch(64)
    _batch_check(capi, oracle, rng, probs, [_same_split(probs[0])] + ([_form("split", 3), _form("shuffle", 4)] if lane == "0" else []),
                 2 if lane == "1" else 1)
    if lane == "1":   # patterns of their own (each lane walks its own)
        _batch_check(capi, oracle, rng, probs[:16], [_form("split", 5)], 2)


@pytest.mark.parametrize("engine", ["0", "1"])
def test_batch_lds_null_space(capi, oracle, monkeypatch, engine):
    monkeypatch.setenv("RSQP_SMALL_ENGINE", engine)
    rng = np.random.default_rng(61)
    probs = [problems.random_qp(rng, int(rng.integers(10, 30)), int(rng.integers(4, 20)), 0.4) for _ in range(12)]
    _batch_check(capi, oracle, rng, probs, [_form("split", 6), _form("shuffle", 7), _form("cancel", 8)], 0)


def test_batch_mid_size_tableau(capi, oracle):
    """members of more than 32 variables: the mid-size tableau kernel (qp_small_g.h) runs first inside the launch of the LDS-resident
    family (rsqp_batch_get_last_kernel 0), for cold starts and hot starts on new vectors"""
    rng = np.random.default_rng(71)
    probs = [problems.random_qp(rng, 40, 20, 0.4) for _ in range(8)]
    _batch_check(capi, oracle, rng, probs, [_form("split", 9), _form("shuffle", 10)], 0)


def test_batch_hbm_small_kernel(capi, oracle):
    rng = np.random.default_rng(81)
    probs = [handler_shaped_qp(rng, 20, 40) for _ in range(6)]
    assert probs[0].nV == 100
    _batch_check(capi, oracle, rng, probs, [_form("split", 11), _form("shuffle", 12)], 3)


# --------------------------------------------------------------------------
# refusals
# --------------------------------------------------------------------------
def test_malformed_csc_is_refused(capi):
    q = problems.random_qp(np.random.default_rng(91), 6, 4, 0.8)
    bad = []
    jc = q.A_jc.copy(); jc[0] = 1; bad.append((jc, q.A_ir, q.A_val))                   # jc[0] != 0
    jc = q.A_jc.copy(); jc[2] = jc[3] + 1; bad.append((jc, q.A_ir, q.A_val))           # decreasing column pointers
    ir = q.A_ir.copy(); ir[0] = q.nC; bad.append((q.A_jc, ir, q.A_val))                # row out of range
    ir = q.A_ir.copy(); ir[0] = -1; bad.append((q.A_jc, ir, q.A_val))
    for A in bad:
        s = capi.Solver(q.nV, q.nC)
        with pytest.raises(capi.RsqpError) as e:
            s.set_A_csc(*A)
        assert e.value.code == capi.ERR_ARG
        s.close()
        b_probs = [q, with_matrices(q, A=A)]
        with pytest.raises(capi.RsqpError) as e:
            capi.Batch(b_probs, device=0)
        assert e.value.code == capi.ERR_ARG
    Hb = []
    jc = q.H_jc.copy(); jc[0] = 1; Hb.append((jc, q.H_ir, q.H_val))
    jc = q.H_jc.copy(); jc[2] = jc[3] + 1; Hb.append((jc, q.H_ir, q.H_val))
    ir = q.H_ir.copy(); ir[0] = q.nV; Hb.append((q.H_jc, ir, q.H_val))
    for H in Hb:
        s = capi.Solver(q.nV, q.nC)
        with pytest.raises(capi.RsqpError) as e:
            s.set_H_csc(*H)
        assert e.value.code == capi.ERR_ARG
        s.close()
        with pytest.raises(capi.RsqpError) as e:
            capi.Batch([with_matrices(q, H=H), q], device=0)
        assert e.value.code == capi.ERR_ARG
