"""numpy restatement of the keyframe pose-graph optimisation: residual, Jacobians, the chain
preconditioner as two prefix sums, preconditioned conjugate gradients over the edges, and the Gauss-Newton loop with its stops.
Poses are 4x4 arrays; a graph's edges are a dict of arrays {"i": (m,), "j": (m,), "Z": (m, 4, 4), "w": (m, 6)}, the first
N - 1 of them the chain.  Tangent order is Sophus' (upsilon, omega).  `solve(..., linear="direct")` replaces the conjugate
gradients by a direct solve of the assembled normal equations: the yardstick the device is held against."""
import numpy as np

STOP_NOT_RUN, STOP_STEP, STOP_ITERATIONS, STOP_COST, STOP_CG_LIMIT = 0, 1, 2, 3, 4
DEFAULTS = dict(max_iterations=30, max_cg_iterations=20000, step_tol=1e-7, cg_tol=1e-10)


def hat(v):
    v = np.asarray(v, float)
    o = np.zeros(v.shape[:-1] + (3, 3))
    o[..., 0, 1], o[..., 0, 2] = -v[..., 2], v[..., 1]
    o[..., 1, 0], o[..., 1, 2] = v[..., 2], -v[..., 0]
    o[..., 2, 0], o[..., 2, 1] = -v[..., 1], v[..., 0]
    return o


def se3_exp(x):
    """(n, 6) -> (n, 4, 4): R = exp(hat(omega)), t = V upsilon"""
    x = np.atleast_2d(np.asarray(x, float))
    u, om = x[:, :3], x[:, 3:]
    th2 = np.sum(om * om, axis=1)
    th = np.sqrt(th2)
    small = th < 1e-6
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)                      # sin(th) / th
    b = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / (ths * ths))     # (1 - cos) / th^2
    c = np.where(small, 1.0 / 6.0 - th2 / 120.0, (ths - np.sin(ths)) / (ths ** 3))
    Om = hat(om)
    Om2 = Om @ Om
    eye = np.eye(3)[None]
    R = eye + a[:, None, None] * Om + b[:, None, None] * Om2
    V = eye + b[:, None, None] * Om + c[:, None, None] * Om2
    T = np.zeros((len(x), 4, 4))
    T[:, :3, :3] = R
    T[:, :3, 3] = np.einsum("nij,nj->ni", V, u)
    T[:, 3, 3] = 1.0
    return T


def se3_log(T):
    """(n, 4, 4) -> (n, 6); rotations away from pi (a residual's are small)"""
    T = np.asarray(T, float).reshape(-1, 4, 4)
    R, t = T[:, :3, :3], T[:, :3, 3]
    w = 0.5 * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)   # sin(th) axis
    s = np.linalg.norm(w, axis=1)
    cth = 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0)
    th = np.arctan2(s, cth)
    small = th < 1e-6
    ss = np.where(small, 1.0, s)
    om = w * np.where(small, 1.0 + th * th / 6.0, th / ss)[:, None]
    ths = np.where(small, 1.0, th)
    c2 = np.where(small, 1.0 / 12.0, (1.0 - ths * np.cos(0.5 * ths) / (2.0 * np.sin(0.5 * ths))) / (ths * ths))
    Om = hat(om)
    Vinv = np.eye(3)[None] - 0.5 * Om + c2[:, None, None] * (Om @ Om)
    return np.concatenate([np.einsum("nij,nj->ni", Vinv, t), om], axis=1)


def inv(T):
    T = np.asarray(T, float)
    o = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    o[..., :3, :3] = Rt
    o[..., :3, 3] = -np.einsum("...ij,...j->...i", Rt, T[..., :3, 3])
    o[..., 3, 3] = 1.0
    return o


def adjoint(T):
    """Ad(T) = [[R, hat(t) R], [0, R]]"""
    T = np.asarray(T, float)
    R, t = T[..., :3, :3], T[..., :3, 3]
    A = np.zeros(T.shape[:-2] + (6, 6))
    A[..., :3, :3] = R
    A[..., 3:, 3:] = R
    A[..., :3, 3:] = hat(t) @ R
    return A


def as_edges(i, j, Z, w):
    return {"i": np.asarray(i, np.int64), "j": np.asarray(j, np.int64), "Z": np.asarray(Z, float).reshape(-1, 4, 4),
            "w": np.asarray(w, float).reshape(-1, 6)}


def residuals(P, E):
    """e = log(Z^-1 P_i^-1 P_j), (m, 6)"""
    P = np.asarray(P, float)
    return se3_log(inv(E["Z"]) @ inv(P[E["i"]]) @ P[E["j"]])


def cost(P, E):
    e = residuals(P, E)
    return float(np.sum(E["w"] * e * e))


def linearise(P, E):
    """e (m, 6), A (m, 6, 6) with J_i = -A, J_j = I"""
    P = np.asarray(P, float)
    return residuals(P, E), adjoint(inv(P[E["j"]]) @ P[E["i"]])


def gather(n, E, at_j, at_i):
    """node sums of the edges' two contributions, in edge order; node 0 is fixed: its row stays 0"""
    y = np.zeros((n, 6))
    np.add.at(y, E["j"], at_j)
    np.add.at(y, E["i"], at_i)
    y[0] = 0.0
    return y


def rhs(n, E, e, A):
    """-J^T W e"""
    g = E["w"] * e
    return gather(n, E, -g, np.einsum("mba,mb->ma", A, g))


def matvec(n, E, A, p):
    """J^T W J p"""
    q = E["w"] * (p[E["j"]] - np.einsum("mab,mb->ma", A, p[E["i"]]))
    return gather(n, E, q, -np.einsum("mba,mb->ma", A, q))


def chain_preconditioner(P, E):
    """r (N, 6) -> M^-1 r with M = J_c^T W_c J_c over the chain edges, as a suffix and a prefix sum (row 0 stays 0)"""
    P = np.asarray(P, float)
    n = len(P)
    Q = inv(P[0])[None] @ P
    AdQ, AdQi = adjoint(Q), adjoint(inv(Q))
    wc = E["w"][: n - 1]

    def apply(r):
        z = np.zeros((n, 6))
        if n < 2:
            return z
        a = np.einsum("nba,nb->na", AdQi[1:], r[1:])           # Ad(Q_k)^-T r_k
        v = np.cumsum(a[::-1], axis=0)[::-1]                     # v_{k-1} = v_k + a_k
        u = np.einsum("nba,nb->na", AdQ[1:], v) / wc             # u_{k-1} = Ad(Q_k)^T v_{k-1}, over the chain weights
        s = np.cumsum(np.einsum("nab,nb->na", AdQ[1:], u), axis=0)   # s_{k+1} = s_k + Ad(Q_{k+1}) u_k
        z[1:] = np.einsum("nab,nb->na", AdQi[1:], s)            # y_k = Ad(Q_k^-1) s_k
        return z
    return apply


def normal_matrix(n, E, A):
    """J^T W J over nodes 1 .. N-1, dense"""
    H = np.zeros((n, 6, n, 6))
    for k in range(len(E["i"])):
        i, j, W, Ak = int(E["i"][k]), int(E["j"][k]), np.diag(E["w"][k]), A[k]
        H[j, :, j, :] += W
        H[i, :, i, :] += Ak.T @ W @ Ak
        H[i, :, j, :] -= Ak.T @ W
        H[j, :, i, :] -= W @ Ak
    return H[1:, :, 1:, :].reshape(6 * (n - 1), 6 * (n - 1))


def chain_matrix(P, E):
    """M assembled densely over nodes 1 .. N-1 (for the check of the prefix form)"""
    n = len(P)
    Ec = {k: v[: n - 1] for k, v in E.items()}
    return normal_matrix(n, Ec, linearise(P, Ec)[1])


def direct_solve(n, E, A, b):
    """the step from the assembled normal equations (sparse when scipy is there, else dense)"""
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
    except ImportError:
        d = np.linalg.solve(normal_matrix(n, E, A), b[1:].reshape(-1))
        return np.concatenate([np.zeros((1, 6)), d.reshape(n - 1, 6)])
    i, j, w = E["i"], E["j"], E["w"]
    WA = w[:, :, None] * A
    blocks = [(j, j, np.einsum("ma,ab->mab", w, np.eye(6))), (i, i, np.einsum("mca,mcb->mab", A, WA)),
              (i, j, -np.swapaxes(WA, 1, 2)), (j, i, -WA)]
    rows, cols, vals = [], [], []
    a6 = np.arange(6)
    for r, c, B in blocks:
        rows.append((6 * r[:, None, None] + a6[None, :, None] + 0 * a6[None, None, :]).reshape(-1))
        cols.append((6 * c[:, None, None] + 0 * a6[None, :, None] + a6[None, None, :]).reshape(-1))
        vals.append(B.reshape(-1))
    H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n)).tocsc()
    d = spl.spsolve(H[6:, 6:], b[1:].reshape(-1))
    return np.concatenate([np.zeros((1, 6)), d.reshape(n - 1, 6)])


def pcg(n, E, A, b, precond, cg_tol, max_cg):
    """-> (x, iterations, sqrt(rz / rz0), ended on the iteration limit)"""
    x = np.zeros((n, 6))
    r = b.copy()
    z = precond(r)
    p = z.copy()
    rz = float(np.sum(r * z))
    rz0 = rz
    it = 0
    limit = False
    while True:
        if not (rz > cg_tol * cg_tol * rz0):
            break
        if it >= max_cg:
            limit = True
            break
        Ap = matvec(n, E, A, p)
        pAp = float(np.sum(p * Ap))
        if not (pAp > 0.0):
            break
        alpha = rz / pAp
        x += alpha * p
        r -= alpha * Ap
        z = precond(r)
        rz_new = float(np.sum(r * z))
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    return x, it, (np.sqrt(rz / rz0) if rz0 > 0 else 0.0), limit


def solve(poses, E, linear="pcg", **cfg):
    """Gauss-Newton as the contract states it -> (poses (N, 4, 4), info)"""
    c = dict(DEFAULTS)
    c.update(cfg)
    P = np.array(poses, float).reshape(-1, 4, 4)
    n, m = len(P), len(E["i"])
    info = dict(n_nodes=n, n_edges=m, n_loop_edges=m - (n - 1), iterations=0, stop_reason=STOP_NOT_RUN, reverted=0,
                cg_iterations=0, initial_cost=0.0, final_cost=0.0, last_step=0.0, last_cg_residual=0.0)
    if n < 2 or m <= n - 1:
        return P, info
    cur = cost(P, E)
    info["initial_cost"] = cur
    limit = False
    for it in range(c["max_iterations"]):
        e, A = linearise(P, E)
        b = rhs(n, E, e, A)
        if linear == "direct":
            d, limit = direct_solve(n, E, A, b), False
        else:
            d, k, rel, limit = pcg(n, E, A, b, chain_preconditioner(P, E), c["cg_tol"], c["max_cg_iterations"])
            info["cg_iterations"] += k
            info["last_cg_residual"] = float(rel)
        Pn = P @ se3_exp(d)
        Pn[0] = P[0]
        new = cost(Pn, E)
        info["iterations"] = it + 1
        info["last_step"] = float(np.max(np.abs(d)))
        small = info["last_step"] < c["step_tol"]   # (a step below step_tol is kept on its size: the cost no longer resolves it)
        if not np.isfinite(new) or (new > cur and not small):
            info["stop_reason"], info["reverted"] = STOP_COST, 1
            break
        P, cur = Pn, new
        if small:
            info["stop_reason"] = STOP_CG_LIMIT if limit else STOP_STEP
            break
    else:
        info["stop_reason"] = STOP_CG_LIMIT if limit else STOP_ITERATIONS
    info["final_cost"] = cur
    return P, info
