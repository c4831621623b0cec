"""The matrices of the QPhandler of every member of a batch on the device (rsqp_batch_handler_set_matrices,
rsqp_batch_get_matrix_values; restartsqp_amd/csrc/rsqp_batch_handler.hip). Expected pools come from handler.batch_matrices_reference (checked
against problems.handler_qp on the CPU, tests/test_batch_handler_matrices_args.py), never from the library. What the pools do not
show -- the CSR copy of A, the update marks, the kernel family -- is checked on twins: two batches of the same members, one driven
through the host setter rsqp_batch_set_matrix_values_of and one through the new call, must dispatch, run and answer alike, byte for
byte (it is the same kernel on the same pools)."""
import numpy as np
import pytest

from restartsqp_amd import problems
from restartsqp_amd.handler import BatchQPhandler, batch_matrices_reference
from restartsqp_amd.qpdump import QPData, dense_to_csc

import test_gpu_batch_handler as G
import test_gpu_batch_members as M

pytestmark = pytest.mark.gpu
T = M.T

# the search route; no constraints (no entry in jac at all); one variable; more slacks than variables
RAGGED = [(4, 2), (3, 1), (5, 0), (1, 1), (2, 3), (4, 2)]


def handler_member(rng, n, m, mask=None, name="synthetic"):
    """a QP of the QPhandler shape: A = [J I -I] with 0.1 <= |J_ij| <= 1 where mask is set (None: everywhere), H = blkdiag(H_k, 0)
    with H_k dense and positive definite; feasible at 0"""
    nV = n + 2 * m
    J = rng.uniform(0.1, 1.0, (m, n)) * rng.choice([-1.0, 1.0], (m, n))
    if mask is not None:
        J = J * mask
    A = np.hstack([J, np.eye(m), -np.eye(m)])
    R = rng.normal(size=(n, n))
    H = np.zeros((nV, nV)); H[:n, :n] = R @ R.T / n + np.eye(n)
    g = np.concatenate([rng.normal(size=n), np.ones(2 * m)])
    lb = np.concatenate([-np.ones(n), np.zeros(2 * m)]); ub = np.concatenate([np.ones(n), np.full(2 * m, 1.0e18)])
    return QPData(nV, m, *dense_to_csc(H), *dense_to_csc(A), g, lb, ub, np.full(m, -0.5), np.full(m, 0.5), name=name)


def ragged_members(rng):
    masks = [rng.random((m, n)) < 0.6 for n, m in RAGGED]
    masks[0][:, 1] = False                            # an empty column
    masks[0][0, 0] = masks[0][1, 2] = True
    masks[5][:, 2] = True                             # a full column
    masks[3][:] = True
    masks[4][:, 0] = True
    return [handler_member(rng, n, m, k) for (n, m), k in zip(RAGGED, masks)]


def open_problem(b):
    """rsqp_batch_handler_set_problem (the shape check of the layer); the NLP bounds play no role for the matrices"""
    sN, sC = b._handler_sizes()
    b.handler_set_problem(np.full(sN, -np.inf), np.full(sN, np.inf), np.full(sC, -np.inf), np.full(sC, np.inf))


def n_of(q):
    return q.nV - 2 * q.nC


def new_entries(rng, q):
    """new J entries (each moved by a few per cent) and new H entries (scaled: as symmetric and as definite as before)"""
    return (q.A_val[:q.A_jc[n_of(q)]] * (1.0 + 0.05 * rng.normal(size=q.A_jc[n_of(q)])),
            None if q.H_val is None else q.H_val * rng.uniform(0.9, 1.2))


def pooled(parts, keep):
    """the members' arrays concatenated, NaN in every entry of a member with keep[q] false: a read of it would show"""
    return M.nan_where(parts, keep)


def send(b, words, jac, hess, on_device):
    words = np.asarray(words, np.int32)
    if not on_device:
        return b.handler_set_matrices(words, jac, hess)
    import torch
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device="cuda")
    args = (t(words, np.int32), t(jac, np.float64), t(hess, np.float64))
    torch.cuda.synchronize()                          # (the inputs are complete before the call)
    b.handler_set_matrices(*args, on_device=True)


class Pools:
    """a batch with the handler layer open, and the value pools the reference expects of it"""

    def __init__(self, capi, members):
        self.capi, self.members = capi, members
        self.b = capi.Batch(members)
        open_problem(self.b)
        self.haveH = members[0].H_jc is not None
        self.A = np.concatenate([q.A_val for q in members] + [np.zeros(0)])
        self.H = np.concatenate([q.H_val for q in members] + [np.zeros(0)]) if self.haveH else None
        self.offA = np.concatenate([[0], np.cumsum(self.b.annz)])
        self.offH = np.concatenate([[0], np.cumsum(self.b.hnnz)]) if self.haveH else None

    def call(self, tag, rng, words, on_device=False):
        """one handler_set_matrices with fresh values for the members the words name; asserts the pools against the reference"""
        capi, b = self.capi, self.b
        J, H = capi.HM_JAC, capi.HM_HESS
        new = [new_entries(rng, q) for q in self.members]
        jac = pooled([e[0] for e in new], [w & J for w in words])
        hess = pooled([e[1] for e in new], [w & H for w in words]) if self.haveH else None
        send(b, words, jac, hess, on_device)
        A2, H2 = batch_matrices_reference(self.A, self.H, words, jac, hess, b.nV, b.nC, [q.A_jc for q in self.members],
                                          [q.H_jc for q in self.members] if self.haveH else None)
        gA, gH = b.get_matrix_values()
        assert gA.tobytes() == A2.tobytes(), (tag, "A", np.flatnonzero(gA != A2)[:8])
        assert (gH is None) == (H2 is None) and (gH is None or gH.tobytes() == H2.tobytes()), (tag, "H")
        assert not np.isnan(gA).any() and (gH is None or not np.isnan(gH).any()), tag
        for q, w in enumerate(words):
            if w == 0:                                # a member with word 0 keeps every byte
                assert gA[self.offA[q]:self.offA[q + 1]].tobytes() == self.A[self.offA[q]:self.offA[q + 1]].tobytes(), (tag, q)
                if self.haveH:
                    assert gH[self.offH[q]:self.offH[q + 1]].tobytes() == self.H[self.offH[q]:self.offH[q + 1]].tobytes(), (tag, q)
        self.A, self.H = A2, H2
        return gA, gH

    def current(self):
        """the members with the values of the pools"""
        out = []
        for q, m in enumerate(self.members):
            Hv = self.H[self.offH[q]:self.offH[q + 1]] if self.haveH else None
            out.append(QPData(m.nV, m.nC, m.H_jc, m.H_ir, Hv, m.A_jc, m.A_ir, self.A[self.offA[q]:self.offA[q + 1]], m.g, m.lb, m.ub,
                              m.lbA, m.ubA, name=m.name))
        return out

    def assert_solves_as_a_fresh_batch(self, tag):
        """a cold rsqp_batch_solve reads nothing but the pools, the CSR copy of A among them: the answers of this batch and of one
        created from the expected values are byte-identical iff what the solve reads is"""
        fresh = self.capi.Batch(self.current())
        self.b.solve(self.capi.MODE_COLD, 1000); fresh.solve(self.capi.MODE_COLD, 1000)
        assert self.b.last_kernel() == fresh.last_kernel(), (tag, self.b.last_kernel(), fresh.last_kernel())
        ra, rc = self.b.results(), fresh.results()
        assert all(M.same_bytes(a, c) for a, c in zip(ra, rc)), (tag, [q for q, (a, c) in enumerate(zip(ra, rc)) if not M.same_bytes(a, c)])
        assert all(r["status"] == 20 for r in ra), (tag, [r["status"] for r in ra])
        fresh.close()


def ragged_schedule(capi):
    J, H = capi.HM_JAC, capi.HM_HESS
    return [[J, H, J | H, 0, J, 0],
            [H, 0, 0, J | H, J | H, J],
            [0, 0, 0, 0, 0, 0],                       # names nobody
            [J | H, J | H, 0, 0, H, H],
            [0, J, H, J, 0, J | H]]


def test_ragged_batch(capi):
    """six members of five shapes, sparse J with an empty and a full column, one member without constraints: the member of an entry
    of jac is searched in the J offsets and of hess in the descriptors. After every call the pools equal the reference"""
    rng = np.random.default_rng(51)
    p = Pools(capi, ragged_members(rng))
    q0, q5 = p.members[0], p.members[5]
    assert q0.A_jc[1] == q0.A_jc[2] and q5.A_jc[3] - q5.A_jc[2] == 2 and p.b.jnz[2] == 0 and 0 < p.b.jnz[0] < 8
    seen = set()
    for k, words in enumerate(ragged_schedule(capi)):
        p.call(("ragged", k), rng, words)
        seen |= set(words)
    assert seen == {0, 1, 2, 3}
    p.assert_solves_as_a_fresh_batch("ragged")
    p.b.close()


def one_pattern_words(capi, call, nq):
    J, H = capi.HM_JAC, capi.HM_HESS
    cycle = [J, 0, H, J | H, 0, J, J | H, H, 0]
    return [0] * nq if call == 2 else [cycle[(q + 4 * call) % len(cycle)] for q in range(nq)]


def run_one_pattern(capi, on_device):
    """300 hs071-shaped members: 2 400 entries in jac, more than nine workgroups of 256 with a partial last one, and the division
    route. Four calls, one of which names nobody; returns the pools after every call"""
    rng = np.random.default_rng(53)
    p = Pools(capi, problems.hs071_scale_batch(300))
    assert p.b.jnz.sum() == 2400 and len(set(p.b.jnz)) == 1
    out = [p.call(("one pattern", on_device, call), rng, one_pattern_words(capi, call, 300), on_device) for call in range(4)]
    p.assert_solves_as_a_fresh_batch(("one pattern", on_device))
    p.b.close()
    return out


def test_one_pattern_batch(capi):
    run_one_pattern(capi, False)


def test_batch_without_h(capi):
    """HESS is ignored and hess may be missing; a word with HESS alone writes nothing and raises nothing"""
    rng = np.random.default_rng(55)
    members = ragged_members(rng)
    for q in members:
        q.H_jc = q.H_ir = q.H_val = None
    p = Pools(capi, members)
    J, H = capi.HM_JAC, capi.HM_HESS
    p.call(("no H", 0), rng, [J | H, H, J, 0, J | H, H])
    p.call(("no H", 1), rng, [H, H, H, H, H, H])
    gA, gH = p.call(("no H", 2), rng, [0, J, J | H, J, H, J])
    assert gH is None
    # the same through the raw entry point, with a hess pointer that must not be read
    w = np.array([H, J | H, 0, 0, 0, 0], np.int32)
    jac = pooled([q.A_val[:q.A_jc[n_of(q)]] * 2.0 for q in members], [0, 1, 0, 0, 0, 0])
    assert capi.lib().rsqp_batch_handler_set_matrices(p.b._h, w.ctypes.data, jac.ctypes.data, None, 0) == capi.OK
    A2, _ = batch_matrices_reference(p.A, None, w, jac, None, p.b.nV, p.b.nC, [q.A_jc for q in members])
    assert p.b.get_matrix_values()[0].tobytes() == A2.tobytes()
    p.b.close()


def test_non_canonical_create_layout(capi):
    """member 0 is created with one J column in descending rows and one position stored twice; member 1 is canonical. The caller's
    layout comes back, and after a solve the answers are those of a batch created canonically from the summed matrices"""
    rng = np.random.default_rng(57)
    a, c = handler_member(rng, 3, 2), handler_member(rng, 4, 2)
    # column 0 in descending rows; position (0, 1) twice, its two values summing to the entry
    v = a.A_val
    ir = np.concatenate([[1, 0], [0, 0, 1], a.A_ir[4:]]).astype(np.int32)
    jc = np.concatenate([a.A_jc[:2], a.A_jc[2:] + 1]).astype(np.int32)
    val = np.concatenate([[v[1], v[0]], [0.5 * v[2], 0.5 * v[2], v[3]], v[4:]])
    u = QPData(a.nV, a.nC, a.H_jc, a.H_ir, a.H_val, jc, ir, val, a.g, a.lb, a.ub, a.lbA, a.ubA, name="folded")
    assert np.array_equal(u.dense_A(), a.dense_A())
    p = Pools(capi, [u, c])
    assert p.b.jnz.tolist() == [7, 8]
    J, H = capi.HM_JAC, capi.HM_HESS
    for k, words in enumerate(([J | H, 0], [H, J], [J, J | H])):
        p.call(("folded", k), rng, words)
    # the canonical twin: the summed entries
    cur = p.current()
    dense = cur[0].dense_A()
    twin0 = QPData(a.nV, a.nC, a.H_jc, a.H_ir, cur[0].H_val, *dense_to_csc(dense), a.g, a.lb, a.ub, a.lbA, a.ubA, name="summed")
    assert np.array_equal(twin0.A_jc, a.A_jc) and np.array_equal(twin0.A_ir, a.A_ir)
    fresh = capi.Batch([twin0, cur[1]])
    p.b.solve(capi.MODE_COLD, 1000); fresh.solve(capi.MODE_COLD, 1000)
    ra, rc = p.b.results(), fresh.results()
    assert p.b.last_kernel() == fresh.last_kernel()
    assert all(M.same_bytes(x, y) for x, y in zip(ra, rc)) and all(r["status"] == 20 for r in ra), [r["status"] for r in ra]
    fresh.close(); p.b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# twins: the host setter on one batch, the new call on the other
# ---------------------------------------------------------------------------------------------------------------------------------
def cat(members, name):
    return np.concatenate([getattr(q, name) for q in members] + [np.zeros(0)])


def assert_twins_alike(tag, x, y, solved_ok=True):
    """after an optimize_qp on both: dispatch, kernel, status, counts, working sets equal, x, y and obj the same bytes"""
    (mx, rx), (my, ry) = x.dispatch(), y.dispatch()
    assert np.array_equal(mx, my) and np.array_equal(rx, ry), (tag, mx, my, rx, ry)
    assert x.last_kernel() == y.last_kernel(), (tag, x.last_kernel(), y.last_kernel())
    a, c = x.results(), y.results()
    assert all(M.same_bytes(p, q) for p, q in zip(a, c)), (tag, [k for k, (p, q) in enumerate(zip(a, c)) if not M.same_bytes(p, q)])
    if solved_ok:
        ok, kkt = y.test_optimality()
        assert all(ok[k] == 1 for k, r in enumerate(c) if r["status"] == 20), (tag, [float(kkt[k]) for k in range(len(c)) if ok[k] != 1])
    return my


def twin_update(capi, x, y, members, words, A2, H2, on_device):
    """the members' new values: on x through rsqp_batch_set_matrix_values_of -- whole A and H of every member with a bit, the old
    values where its word does not name the matrix --, on y through the new call"""
    J, H = capi.HM_JAC, capi.HM_HESS
    named = [w != 0 for w in words]
    x.set_matrix_values(pooled([a if w & J else q.A_val for q, a, w in zip(members, A2, words)], named),
                        pooled([h if w & H else q.H_val for q, h, w in zip(members, H2, words)], named), members=named)
    send(y, words, pooled([a[:q.A_jc[n_of(q)]] for q, a in zip(members, A2)], [w & J for w in words]),
         pooled(H2, [w & H for w in words]), on_device)
    for q, a, h, w in zip(members, A2, H2, words):     # what the batches hold from here on
        if w & J:
            q.A_val = a
        if w & H:
            q.H_val = h


def new_matrices(rng, members):
    """new A of every member that differs in the J block alone, new H scaled"""
    A2 = []
    for q in members:
        a = q.A_val.copy()
        k = q.A_jc[n_of(q)]
        a[:k] *= 1.0 + 0.01 * rng.normal(size=k)
        A2.append(a)
    return A2, [q.H_val * 1.05 for q in members]


def run_twins(capi, on_device):
    """T.BATCHES["hs64_small"]: 64 members of at most 8 variables in shapes of their own, on the hs071-scale tableau kernel. Returns
    the pools of the batch driven through the new call"""
    rng = np.random.default_rng(59)
    members = T.BATCHES["hs64_small"][0]()
    nq = len(members)
    x, y = capi.Batch(members), capi.Batch(members)
    open_problem(y)
    x.optimize_qp(); y.optimize_qp()
    assert_twins_alike("first", x, y)
    J, H = capi.HM_JAC, capi.HM_HESS
    words = rng.choice([0, 0, J, H, J | H], nq)
    assert set(words.tolist()) == {0, J, H, J | H}
    A2, H2 = new_matrices(rng, members)
    twin_update(capi, x, y, members, words, A2, H2, on_device)
    pools = y.get_matrix_values()
    assert pools[0].tobytes() == cat(members, "A_val").tobytes() and pools[1].tobytes() == cat(members, "H_val").tobytes()
    step = [problems.perturb(rng, q, 0.05) for q in members]
    x.set_vectors_from(step); y.set_vectors_from(step)
    x.optimize_qp(); y.optimize_qp()
    mode = assert_twins_alike("second", x, y)
    assert y.last_kernel() == 1
    # (the marks: a hot start on new matrices for the named members whose first QP was solved, on new vectors for the others)
    assert (mode[words != 0] == capi.MODE_HOT_MATRICES).sum() >= 16 and (mode[words == 0] == capi.MODE_HOT_VECTORS).sum() >= 8, mode
    assert not np.any(mode[words == 0] == capi.MODE_HOT_MATRICES)
    x.close(); y.close()
    return pools


def test_twins_csr_copy_marks_and_family(capi):
    run_twins(capi, False)


def test_family_change_through_the_device_verdict(capi):
    """member 0's H made unsymmetric in one off-diagonal pair moves both twins off the tableau kernel (1 -> 0) and the others' hot
    starts run cold; the host's record of the verdict is what a following host setter for member 1 alone relies on; member 0
    symmetric again through the new call -- on both twins, one of which examined it on the host before -- brings both back"""
    rng = np.random.default_rng(61)
    members = T.BATCHES["hs64_small"][0]()
    nq = len(members)
    x, y = capi.Batch(members), capi.Batch(members)
    open_problem(x); open_problem(y)
    x.optimize_qp(); y.optimize_qp()
    assert_twins_alike("a", x, y)
    assert y.last_kernel() == 1
    q0 = members[0]
    Hd = q0.dense_H()
    r, c = [(i, j) for j in range(q0.nV) for i in range(j + 1, q0.nV) if Hd[i, j] != 0.0][0]
    Hval = [q.H_val.copy() for q in members]
    for k in range(q0.H_jc[c], q0.H_jc[c + 1]):
        if q0.H_ir[k] == r:
            Hval[0][k] *= 1.0 + 1e-3
    only0 = np.arange(nq) == 0
    x.set_matrix_values(None, pooled(Hval, only0), members=only0)
    y.handler_set_matrices(np.where(only0, capi.HM_HESS, 0), None, pooled(Hval, only0))

    def step(tag, kernel):
        nonlocal members
        members = [problems.perturb(rng, q, 0.05) for q in members]
        x.set_vectors_from(members); y.set_vectors_from(members)
        x.optimize_qp(); y.optimize_qp()
        mode = assert_twins_alike(tag, x, y)
        assert x.last_kernel() == y.last_kernel() == kernel, (tag, x.last_kernel(), y.last_kernel())
        return mode

    assert np.all(step("b", 0) == 0)                   # (hot starts on the tableau kernel's states run cold)
    only1 = np.arange(nq) == 1
    for b in (x, y):
        b.set_matrix_values(pooled([q.A_val for q in members], only1), pooled([q.H_val for q in members], only1), members=only1)
    mode = step("c", 0)
    # (member 1 ran on fixed matrices in step b: new ones are a FIXED -> VARIED flip, mode 3; behind a first solve they are mode 2)
    assert int(mode[1]) in (capi.MODE_HOT_MATRICES, capi.MODE_WARM_REINIT) and int(mode[3]) == capi.MODE_HOT_VECTORS, mode[:4]
    for b in (x, y):
        b.handler_set_matrices(np.where(only0, capi.HM_HESS, 0), None, pooled([q.H_val for q in members], only0))
    assert np.all(step("d", 1) == 0)
    mode = step("e", 1)
    assert int(mode[3]) == capi.MODE_HOT_VECTORS, mode[:4]
    x.close(); y.close()


def test_hbm_resident_batch(capi):
    """three members of (n, m) = (96, 2): new J and H for member 1 alone, against a twin driven through the host setter"""
    rng = np.random.default_rng(63)
    members = [handler_member(rng, 96, 2, rng.random((2, 96)) < 0.5) for _ in range(3)]
    x, y = capi.Batch(members), capi.Batch(members)
    open_problem(y)
    x.optimize_qp(); y.optimize_qp()
    assert_twins_alike("first", x, y)
    assert y.last_kernel() == 3
    A2, H2 = new_matrices(rng, members)
    J, H = capi.HM_JAC, capi.HM_HESS
    twin_update(capi, x, y, members, [0, J | H, 0], A2, H2, False)
    pools = y.get_matrix_values()
    assert pools[0].tobytes() == cat(members, "A_val").tobytes() and pools[1].tobytes() == cat(members, "H_val").tobytes()
    step = [problems.perturb(rng, q, 0.05) for q in members]
    x.set_vectors_from(step); y.set_vectors_from(step)
    x.optimize_qp(); y.optimize_qp()
    mode = assert_twins_alike("second", x, y)
    assert mode.tolist() == [1, 2, 1] and y.last_kernel() == 3, (mode, y.last_kernel())
    x.close(); y.close()


def test_lockstep_replay_with_the_matrices_through_the_handler(capi, oracle):
    """test_gpu_batch_handler.test_lockstep_replay_through_the_handler with the matrices through BatchQPhandler as well: set_A /
    set_H at a member's first step, update_A / update_H where its trace entry's flags say A or H. One flush sends the matrices,
    then the vectors; both sets of pools must equal problems.handler_qp's for every participant, and the same criteria hold"""
    runs = {name: M.trajectory_qps(name) for name in M.NLPS}
    M.assert_oracle_replays_the_trajectories(oracle, runs)
    nq = len(M.LOCKSTEP)
    b = capi.Batch([runs[name][1][0] for name, start in M.LOCKSTEP])
    nlp0 = [M.NLPS[name]() for name, start in M.LOCKSTEP]
    ns, ms = [p["info"].nVar for p in nlp0], [p["info"].nCon for p in nlp0]
    offN, offC = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(ms)])
    offA, offH = np.concatenate([[0], np.cumsum(b.annz)]), np.concatenate([[0], np.cumsum(b.hnnz)])
    h = BatchQPhandler(b, *[G.cat([p[k] for p in nlp0]) for k in ("x_l", "x_u", "c_l", "c_u")])
    nsteps = max(start + len(runs[name][0]) for name, start in M.LOCKSTEP)
    ties = [0] * nq
    sent = 0
    for t in range(nsteps):
        entry = [t - start if 0 <= t - start < len(runs[name][0]) else None for name, start in M.LOCKSTEP]
        take = np.array([e is not None for e in entry])
        gold = [runs[name][0][e] if e is not None else None for (name, start), e in zip(M.LOCKSTEP, entry)]
        members = [runs[name][1][e if e is not None else 0] for (name, start), e in zip(M.LOCKSTEP, entry)]
        first = np.array([e == 0 for e in entry])
        newA = np.array([g is not None and bool(g["flags"]["A"]) for g in gold]) | first
        newH = np.array([g is not None and bool(g["flags"]["H"]) for g in gold]) | first
        jac = [q.A_val[:q.A_jc[n_of(q)]] for q in members]
        if (newA & first).any():
            h.set_A(newA & first, pooled(jac, newA & first))
        if (newA & ~first).any():
            h.update_A(newA & ~first, pooled(jac, newA & ~first))
        if (newH & first).any():
            h.set_H(newH & first, pooled([q.H_val for q in members], newH & first))
        if (newH & ~first).any():
            h.update_H(newH & ~first, pooled([q.H_val for q in members], newH & ~first))
        for j, ((name, start), g) in enumerate(zip(M.LOCKSTEP, gold)):
            if g is not None:
                G.drive(h, nq, j, g["flags"], M.NLPS[name](np.array(g["x"]), np.array(g["lam"])), g["delta"], g["rho"], offN, offC)
        pools_before, mats_before = b.get_vectors(), b.get_matrix_values()
        words = h.flush()
        assert np.array_equal(words != 0, take), (t, words)
        assert np.array_equal(h.matrix_words, newA * capi.HM_JAC + newH * capi.HM_HESS), (t, h.matrix_words)
        sent += int(h.matrix_words.any())
        pools, mats = b.get_vectors(), b.get_matrix_values()
        for j, (q, g) in enumerate(zip(members, gold)):
            for k, name in enumerate(G.VEC):
                lo, hi = (b.offV[j], b.offV[j + 1]) if k < 3 else (b.offC[j], b.offC[j + 1])
                if g is None:
                    assert pools[k][lo:hi].tobytes() == pools_before[k][lo:hi].tobytes(), (t, j, name)
                else:
                    assert np.array_equal(pools[k][lo:hi], getattr(q, name)), (t, j, name)
            for k, (name, off) in enumerate((("A_val", offA), ("H_val", offH))):
                lo, hi = off[j], off[j + 1]
                if g is None:
                    assert mats[k][lo:hi].tobytes() == mats_before[k][lo:hi].tobytes(), (t, j, name)
                else:                                 # (a matrix whose flag is not set has not changed along the trace)
                    assert mats[k][lo:hi].tobytes() == getattr(q, name).tobytes(), (t, j, name)
        before = b.results()
        used, ok, kkt = h.solveQP(take)
        assert b.last_kernel() == 0
        mode, rescue = b.dispatch()
        res = b.results()
        st = h.step()
        for j, ((name, start), g) in enumerate(zip(M.LOCKSTEP, gold)):
            tag = (name, j, t)
            if g is None:
                M.assert_sitter(tag, before[j], res[j], used[j], mode[j], rescue[j])
                continue
            r = res[j]
            assert int(mode[j]) == T.MODES[g["mode"]] and int(rescue[j]) == 0, (tag, int(mode[j]), g["mode"], int(rescue[j]))
            assert r["status"] == g["status"] == 20, (tag, r["status"])
            assert ok[j] == 1, (tag, float(kkt[j]))
            gx, gy = np.array(g["x_qp"]), np.array(g["y_qp"])
            tol = 1e-9 * max(1.0, np.abs(gx).max())
            assert np.abs(r["x"] - gx).max() <= tol, (tag, g["mode"])
            assert abs(r["obj"] - g["obj"]) <= 1e-9 * max(1.0, abs(g["obj"])), tag
            assert np.abs(st["p"][offN[j]:offN[j + 1]] - gx[:ns[j]]).max() <= tol, tag
            assert abs(st["infea_model"][j] - np.abs(gx[ns[j]:]).sum()) <= tol, (tag, float(st["infea_model"][j]))
            same_path = int(used[j]) == g["nWSR"] and np.array_equal(r["ws_b"], g["ws_b"]) and np.array_equal(r["ws_c"], g["ws_c"])
            if name == "hs065":
                ties[j] += not same_path
                continue
            assert same_path, (tag, g["mode"], int(used[j]), g["nWSR"])
            assert np.abs(r["y"] - gy).max() <= 1e-9 * max(1.0, np.abs(gy).max()), (tag, g["mode"])
    assert max(ties) <= 3, ties
    assert sent >= nsteps // 2, (sent, nsteps)          # (condition on the inputs: most steps bring a matrix)
    b.close()


def test_call_order_and_shape_errors(capi):
    """a call before rsqp_batch_handler_set_problem, a word that names a matrix that is not given (host pointers) and a missing what
    give RSQP_ERR_ARG; a what of the wrong length cannot be seen by the library, which gets a bare pointer: the binding refuses it
    (ValueError) before the library is reached. The pools are unchanged after all of them"""
    rng = np.random.default_rng(65)
    members = ragged_members(rng)
    b = capi.Batch(members)
    J, H = capi.HM_JAC, capi.HM_HESS
    before = b.get_matrix_values()
    new = [new_entries(rng, q) for q in members]
    jac, hess = pooled([e[0] for e in new], [1] * 6), pooled([e[1] for e in new], [1] * 6)
    with pytest.raises(capi.RsqpError) as e:            # before rsqp_batch_handler_set_problem
        b.handler_set_matrices([J | H] * 6, jac, hess)
    assert e.value.code == capi.ERR_ARG
    open_problem(b)
    L = capi.lib()
    w = np.array([J, 0, H, 0, 0, 0], np.int32)
    # a word names a matrix that is not given (host pointers); the binding refuses it too, so through the raw entry point
    assert L.rsqp_batch_handler_set_matrices(b._h, w.ctypes.data, None, hess.ctypes.data, 0) == capi.ERR_ARG
    assert L.rsqp_batch_handler_set_matrices(b._h, w.ctypes.data, jac.ctypes.data, None, 0) == capi.ERR_ARG
    assert L.rsqp_batch_handler_set_matrices(b._h, None, jac.ctypes.data, hess.ctypes.data, 0) == capi.ERR_ARG
    assert b"rsqp_batch_handler_set_matrices" in L.rsqp_last_error()
    with pytest.raises(ValueError):
        b.handler_set_matrices(w, None, hess)
    for bad in (np.zeros(5, np.int32), np.zeros(7, np.int32)):      # a what of the wrong length never reaches the library
        with pytest.raises(ValueError):
            b.handler_set_matrices(bad, jac, hess)
    after = b.get_matrix_values()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))      # (nothing was written)
    b.close()


def test_device_pointers():
    """the one-pattern case and the twins with what, jac and hess as torch tensors on the device, and a BatchQPhandler(on_device=True)
    flush with matrices and vectors pending, against the host-pointer runs. In a child process that imports torch BEFORE the library
    is loaded (tests/checks/handler_matrices_device_pointers.py)"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "handler_matrices_device_pointers.py")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "HANDLER MATRICES DEVICE POINTERS OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
