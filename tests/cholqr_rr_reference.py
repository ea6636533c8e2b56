"""numpy restatement of the staged rank-revealing Cholesky-QR (FEASTHIP_ORTHO_CHOLQR_RR): fh_cholqr::pivoted_stage
(csrc/fh_cholqr.hpp), k_pchol_stage (csrc/fh_blockops.hip) and the stage loop of fh_ortho_staged (csrc/fh_ortho.hip), with the
same stages, window and stop rule.  The rank rule is that of _feast_qr_compress! (src/core/feast_aux.jl:101-131)."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
WINDOW = 1e-10          # FH_RR_WINDOW: ratio of squared pivots one stage may span
MAX_STAGES = 6          # FH_RR_MAX_STAGES


def threshold(rank_tol, N, m, big_dim=0):
    return max(rank_tol, EPS * max(N, big_dim, m))


def pivoted_stage(G, alive, window, stop_rel, ref_scale, r11):
    """One stage on the Gram matrix G of the working panel.  alive: columns not decided yet.  r11 None: first stage.
    -> dict(ord, rdiag, done, fail, r11, Rinv) with X @ Rinv the accepted columns after the first pass."""
    G = np.asarray(G)
    G = np.array(G, dtype=complex) if np.iscomplexobj(G) and np.any(G.imag != 0) else np.array(G.real, dtype=float)
    ld = G.shape[0]
    alive = np.asarray(alive, dtype=bool)
    out = dict(ord=[], rdiag=[], done=False, fail=False, r11=r11, Rinv=np.zeros((ld, 0), dtype=G.dtype))
    idx = np.flatnonzero(alive)
    if not np.all(np.isfinite(G[np.ix_(idx, idx)])):
        out["fail"] = out["done"] = True
        return out
    d = np.ones(ld)
    g = G.diagonal().real
    d[alive] = np.where(g[alive] > 0, np.sqrt(np.where(g[alive] > 0, g[alive], 0.0)), 0.0)
    dref = d[alive].max() if idx.size else 0.0
    pos = alive & (d > 0)
    pi = np.flatnonzero(pos)
    G[np.ix_(pi, pi)] = G[np.ix_(pi, pi)] / np.outer(d[pi], d[pi])
    w = np.zeros(ld)
    w[pos] = (d[pos] / dref) ** 2
    if r11 is None:
        r11 = max(dref, ref_scale)
    out["r11"] = r11
    stop = stop_rel * r11
    key = np.where(alive, w * G.diagonal().real, -1.0)
    picked = np.zeros(ld, dtype=bool)
    key0 = 0.0
    order, rdiag = [], []
    while True:
        cand = np.flatnonzero(alive & ~picked)
        if cand.size == 0:
            break
        p = cand[np.argmax(key[cand])]            # first maximum: the lowest index among equals
        best = key[p]
        rkk = dref * np.sqrt(best) if best >= 0 else np.nan
        if not (rkk > stop) or rkk == 0.0:
            out["done"] = True
            break
        if not order:
            key0 = best
        elif not (best > window * key0):
            break
        r = np.sqrt(G[p, p].real)
        order.append(int(p))
        rdiag.append(float(rkk))
        picked[p] = True
        rest = np.flatnonzero(alive & ~picked)
        G[rest, p] = G[rest, p] / r
        G[p, p] = r
        L = G[rest, p]
        G[np.ix_(rest, rest)] -= np.outer(L, L.conj())
        key[rest] = w[rest] * G.diagonal().real[rest]
    k = len(order)
    out["ord"], out["rdiag"] = order, rdiag
    if k == 0:
        if not out["done"]:
            out["fail"] = out["done"] = True
        return out
    o = np.array(order)
    R = np.triu(G[np.ix_(o, o)].conj().T, 1) + np.diag(G.diagonal().real[o])
    Ri = np.linalg.solve(R, np.eye(k))                       # triangular: back substitution
    Rinv = np.zeros((ld, k), dtype=G.dtype)
    Rinv[o, :] = Ri / d[o][:, None]
    out["Rinv"] = Rinv
    return out


def staged_qr(X, rank_tol, ref_scale=0.0, big_dim=0, window=WINDOW, max_stages=MAX_STAGES):
    """The staged factorisation of the panel X (N x m).  -> dict(rank, perm, rdiag, stages, Q, fell_back)."""
    N, m = X.shape
    thr = threshold(rank_tol, N, m, big_dim)
    colmax = float(np.sqrt((np.abs(X) ** 2).sum(axis=0).max())) if m else 0.0
    scale = 2.0 ** -int(np.floor(np.log2(colmax))) if colmax > 0 and np.isfinite(colmax) else 1.0    # exact: a power of two
    W = np.array(X, dtype=complex) * scale
    ref_scale = ref_scale * scale
    Q = np.zeros((N, 0), dtype=complex)
    decided = np.zeros(m, dtype=bool)
    perm, rdiag, r11, stages, done = [], [], None, 0, False
    give_up = dict(rank=0, perm=[], rdiag=[], stages=stages, Q=None, fell_back=True)
    for s in range(max_stages):
        st = pivoted_stage(W.conj().T @ W, ~decided, window, thr, ref_scale, r11)
        if st["fail"]:
            return give_up
        r11 = st["r11"]
        T = W @ st["Rinv"]
        if s > 0:
            T = T - Q @ (Q.conj().T @ T)
        k = len(st["ord"])
        rd = list(st["rdiag"])
        if k:
            G2 = T.conj().T @ T
            try:
                R2 = np.linalg.cholesky(G2).conj().T
            except np.linalg.LinAlgError:
                return give_up
            T2 = T @ np.linalg.solve(R2, np.eye(k))
            rd = [a * b for a, b in zip(rd, R2.diagonal().real)]
            Q = np.hstack([Q, T2])
            decided[st["ord"]] = True
            perm += st["ord"]
            rdiag += rd
        stages += 1
        if st["done"] or len(perm) >= m:
            done = True
            break
        for _ in range(2):
            W = W - T2 @ (T2.conj().T @ W)
    if not done:
        return give_up
    return dict(rank=len(perm), perm=perm, rdiag=[v / scale for v in rdiag], stages=stages, Q=Q, fell_back=False)
