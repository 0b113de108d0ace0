"""numpy restatement of include/ssf_graph_solve.h: the embedded-deformation solve over the resident graph, every step one IEEE f64
operation in the header's order, so the GPU results are compared with it bit for bit.  Below it, direct_gauss_newton: an independent
Gauss-Newton on the same energy (scipy sparse J, a direct solve of every step's normal equations) that the restatement is proven
against; it shares no code with the restatement."""
import numpy as np

import graph_ref as gr

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64
MAX_OUTER = 64
END_TOL, END_MAX_INNER, END_BREAKDOWN, END_ZERO = 0, 1, 2, 3

DEFAULTS = dict(w_rot=1.0, w_reg=10.0, w_con=100.0, max_outer=8, max_inner=512, inner_check=16, inner_tol=1e-6, outer_tol=1e-6,
                damping=0.0)


def nearest5(points, t_init, node_pos, node_t, look):
    """steps 1-4 of ssf_graph.h's binding: k_0 ... k_4 for every point (n x 5 i32)"""
    pos = np.ascontiguousarray(points, f32).reshape(-1, 3)
    t0 = np.asarray(t_init, np.int32).ravel()
    npos = np.ascontiguousarray(node_pos, f32).reshape(-1, 3)
    nt0 = np.asarray(node_t, np.int32).ravel()
    m, L = len(npos), int(look)
    W = min(m, 2 * L)
    c = np.searchsorted(nt0, t0, side="left")
    lo = np.clip(c - L, 0, max(0, m - 2 * L))
    k = lo[:, None] + np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        d = pos[:, None, :] - npos[k]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    key = np.sort((d2.view(u32).astype(u64) << u64(32)) | k.astype(u64), axis=1)[:, :5]
    return (key & u64(0xFFFFFFFF)).astype(np.int32)


def edges_of(node_pos, node_t, look):
    """N(j): the first four of k_0 ... k_4 of node j's own binding that are != j (m x 4 i32); edge id = 4 j + n"""
    k5 = nearest5(node_pos, node_t, node_pos, node_t, look)
    m = len(k5)
    out = np.empty((m, 4), np.int32)
    for j in range(m):
        out[j] = [k for k in k5[j] if k != j][:4]
    return out


def tree_sum(v):
    """blocks of 256 by the halving tree s[i] += s[i + h], h = 128 ... 1, the tail padded with +0.0; block sums added in ascending order
    from +0.0"""
    v = np.asarray(v, f64)
    nb = (len(v) + 255) // 256
    s = np.zeros(nb * 256, f64)
    s[:len(v)] = v
    s = s.reshape(nb, 256)
    h = 128
    while h >= 1:
        s[:, :h] = s[:, :h] + s[:, h:2 * h]
        h //= 2
    tot = f64(0.0)
    for b in range(nb):
        tot = tot + s[b, 0]
    return tot


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def left_sum(cols):
    s = cols[0]
    for c in cols[1:]:
        s = s + c
    return s


def _transposed(keys, m):
    """stable counting sort of the item ids by key: (order, offsets m + 1)"""
    order = np.argsort(keys, kind="stable")
    off = np.searchsorted(keys[order], np.arange(m + 1), side="left")
    return order, off


class Problem:
    def __init__(self, node_pos, node_t, look, src, t_init, dst, **params):
        self.p = dict(DEFAULTS); self.p.update(params)
        npos = np.ascontiguousarray(node_pos, f32).reshape(-1, 3)
        src = np.ascontiguousarray(src, f32).reshape(-1, 3)
        dst = np.ascontiguousarray(dst, f32).reshape(-1, 3)
        self.m, self.nc = len(npos), len(src)
        self.g = npos.astype(f64)
        self.edges = edges_of(npos, node_t, look)
        self.ev = self.g[self.edges] - self.g[:, None, :]                       # e = g_k - g_j
        w4, idx4 = gr.bind(src, t_init, npos, node_t, look)[:2]
        self.idx4, self.w = idx4, w4.astype(f64)
        self.u = src.astype(f64)[:, None, :] - self.g[idx4]                    # u_n = s - g_k
        self.d = dst.astype(f64)
        self.sr, self.sg, self.sc = (np.sqrt(f64(self.p[k])) for k in ("w_rot", "w_reg", "w_con"))
        self.se = self.sg * self.ev                                             # m x 4 x 3
        self.sw = self.sc * self.w                                              # nc x 4
        self.su = self.sw[..., None] * self.u                                   # nc x 4 x 3
        self.in_order, self.in_off = _transposed(self.edges.ravel(), self.m)
        self.con_order, self.con_off = _transposed(self.idx4.ravel(), self.m)

    # ---- residuals and energy ------------------------------------------------------------------------------------------
    def residuals(self, x):
        A, t = x[:, :9].reshape(-1, 3, 3), x[:, 9:]
        c0, c1, c2 = A[:, :, 0], A[:, :, 1], A[:, :, 2]
        sr, sg, sc = self.sr, self.sg, self.sc
        r_rot = np.stack([sr * dot3(c0, c1), sr * dot3(c0, c2), sr * dot3(c1, c2), sr * (dot3(c0, c0) - 1.0),
                          sr * (dot3(c1, c1) - 1.0), sr * (dot3(c2, c2) - 1.0)], 1)
        r_reg = np.empty((self.m, 4, 3), f64)
        for n in range(4):
            k, e = self.edges[:, n], self.ev[:, n]
            Ae = (A[:, :, 0] * e[:, None, 0] + A[:, :, 1] * e[:, None, 1]) + A[:, :, 2] * e[:, None, 2]
            r_reg[:, n] = sg * ((((Ae + self.g) + t) - self.g[k]) - t[k])
        v = []
        for n in range(4):
            k, u = self.idx4[:, n], self.u[:, n]
            Ak = A[k]
            Au = (Ak[:, :, 0] * u[:, None, 0] + Ak[:, :, 1] * u[:, None, 1]) + Ak[:, :, 2] * u[:, None, 2]
            v.append(self.w[:, n, None] * (((Au + self.g[k]) + t[k]) - self.d))
        r_con = sc * (((v[0] + v[1]) + v[2]) + v[3])
        return r_rot, r_reg, r_con

    def energy(self, r):
        r_rot, r_reg, r_con = r
        e_rot = tree_sum(left_sum([r_rot[:, i] * r_rot[:, i] for i in range(6)]))
        rr = r_reg.reshape(self.m, 12)
        e_reg = tree_sum(left_sum([rr[:, i] * rr[:, i] for i in range(12)]))
        e_con = tree_sum(left_sum([r_con[:, i] * r_con[:, i] for i in range(3)]))
        return (e_rot + e_reg) + e_con, e_rot, e_reg, e_con

    # ---- J v, J^T y, diag(J^T J) at x ------------------------------------------------------------------------------------
    def scaled_cols(self, x):
        A = x[:, :9].reshape(-1, 3, 3)
        return self.sr * A[:, :, 0], self.sr * A[:, :, 1], self.sr * A[:, :, 2]

    def J(self, x, v):
        P, pt = v[:, :9].reshape(-1, 3, 3), v[:, 9:]
        s0, s1, s2 = self.scaled_cols(x)
        P0, P1, P2 = P[:, :, 0], P[:, :, 1], P[:, :, 2]
        y_rot = np.stack([dot3(s1, P0) + dot3(s0, P1), dot3(s2, P0) + dot3(s0, P2), dot3(s2, P1) + dot3(s1, P2),
                          dot3(2.0 * s0, P0), dot3(2.0 * s1, P1), dot3(2.0 * s2, P2)], 1)
        y_reg = np.empty((self.m, 4, 3), f64)
        for n in range(4):
            k, se = self.edges[:, n], self.se[:, n]
            Pe = (se[:, None, 0] * P[:, :, 0] + se[:, None, 1] * P[:, :, 1]) + se[:, None, 2] * P[:, :, 2]
            y_reg[:, n] = (Pe + self.sg * pt) - self.sg * pt[k]
        tn = []
        for n in range(4):
            k, su = self.idx4[:, n], self.su[:, n]
            Pk = P[k]
            Pu = (su[:, None, 0] * Pk[:, :, 0] + su[:, None, 1] * Pk[:, :, 1]) + su[:, None, 2] * Pk[:, :, 2]
            tn.append(Pu + self.sw[:, n, None] * pt[k])
        y_con = ((tn[0] + tn[1]) + tn[2]) + tn[3]
        return y_rot, y_reg, y_con

    def _gather(self, accA, acct, own_A, own_t, in_t, con_A, con_t):
        """the per-node sum in the header's order: accA / acct hold the rot rows' share; own_*(n), in_t(edge ids), con_*(incidences)"""
        for n in range(4):
            accA += own_A(n); acct += own_t(n)
        deg = np.diff(self.in_off)
        for r in range(int(deg.max()) if len(deg) else 0):
            nodes = np.flatnonzero(deg > r)
            acct[nodes] += in_t(self.in_order[self.in_off[nodes] + r])
        deg = np.diff(self.con_off)
        for r in range(int(deg.max()) if len(deg) else 0):
            nodes = np.flatnonzero(deg > r)
            inc = self.con_order[self.con_off[nodes] + r]
            accA[nodes] += con_A(inc // 4, inc % 4); acct[nodes] += con_t(inc // 4, inc % 4)
        return np.concatenate([accA.reshape(self.m, 9), acct], 1)

    def Jt(self, x, y):
        y_rot, y_reg, y_con = y
        s0, s1, s2 = self.scaled_cols(x)
        y0, y1, y2, y3, y4, y5 = (y_rot[:, i, None] for i in range(6))
        accA = np.zeros((self.m, 3, 3), f64); acct = np.zeros((self.m, 3), f64)
        accA[:, :, 0] += (y0 * s1 + y1 * s2) + y3 * (2.0 * s0)
        accA[:, :, 1] += (y0 * s0 + y2 * s2) + y4 * (2.0 * s1)
        accA[:, :, 2] += (y1 * s0 + y2 * s1) + y5 * (2.0 * s2)
        yr = y_reg.reshape(-1, 3)
        return self._gather(accA, acct,
                            lambda n: y_reg[:, n, :, None] * self.se[:, n, None, :], lambda n: y_reg[:, n] * self.sg,
                            lambda e: -(yr[e] * self.sg),
                            lambda c, n: y_con[c][:, :, None] * self.su[c, n][:, None, :], lambda c, n: y_con[c] * self.sw[c, n][:, None])

    def diag(self, x):
        s0, s1, s2 = self.scaled_cols(x)
        accA = np.zeros((self.m, 3, 3), f64); acct = np.zeros((self.m, 3), f64)
        accA[:, :, 0] += (s1 * s1 + s2 * s2) + (2.0 * s0) * (2.0 * s0)
        accA[:, :, 1] += (s0 * s0 + s2 * s2) + (2.0 * s1) * (2.0 * s1)
        accA[:, :, 2] += (s0 * s0 + s1 * s1) + (2.0 * s2) * (2.0 * s2)
        sg2 = self.sg * self.sg
        ones = np.ones((1, 3), f64)
        return self._gather(accA, acct,
                            lambda n: np.broadcast_to((self.se[:, n] * self.se[:, n])[:, None, :], (self.m, 3, 3)),
                            lambda n: sg2 * np.ones((self.m, 3), f64),
                            lambda e: sg2 * np.ones((len(e), 3), f64),
                            lambda c, n: np.broadcast_to((self.su[c, n] * self.su[c, n])[:, None, :], (len(c), 3, 3)),
                            lambda c, n: (self.sw[c, n] * self.sw[c, n])[:, None] * ones)

    def dot(self, a, b):
        return tree_sum(left_sum([a[:, c] * b[:, c] for c in range(12)]))

    # ---- the solve ------------------------------------------------------------------------------------------------------
    def pcg(self, x, b, D):
        p_ = self.p
        damping = f64(p_["damping"])
        with np.errstate(all="ignore"):
            inv = lambda r: np.where(D > 0, r / D, 0.0)
            delta = np.zeros_like(b); r = b.copy(); z = inv(r)
            rho0 = rho = self.dot(r, z)
            if not rho0 > 0:
                return delta, 0, END_ZERO
            it, p, rho_prev = 0, None, None
            while True:
                p = z.copy() if it == 0 else z + (rho / rho_prev) * p
                q = self.Jt(x, self.J(x, p)) + damping * p
                pq = self.dot(p, q)
                if not (pq > 0 and np.isfinite(pq)):
                    return delta, it, END_BREAKDOWN
                alpha = rho / pq
                delta = delta + alpha * p
                r = r - alpha * q
                z = inv(r)
                rho_prev, rho = rho, self.dot(r, z)
                it += 1
                if it % p_["inner_check"] == 0 and rho <= (f64(p_["inner_tol"]) * f64(p_["inner_tol"])) * rho0:
                    return delta, it, END_TOL
                if it >= p_["max_inner"]:
                    return delta, it, END_MAX_INNER

    def solve(self):
        p_ = self.p
        x = np.zeros((self.m, 12), f64)
        x[:, 0] = x[:, 4] = x[:, 8] = 1.0
        r = self.residuals(x)
        E = self.energy(r)
        res = dict(outer=0, inner=[], inner_end=END_ZERO, e_before=E[0])
        for _ in range(int(p_["max_outer"])):
            b = -self.Jt(x, r)
            D = self.diag(x) + f64(p_["damping"])
            delta, it, end = self.pcg(x, b, D)
            x = x + delta
            r = self.residuals(x)
            En = self.energy(r)
            res["outer"] += 1; res["inner"].append(it); res["inner_end"] = end
            done = abs(E[0] - En[0]) <= f64(p_["outer_tol"]) * E[0]
            E = En
            if done:
                break
        res.update(e_after=E[0], e_rot=E[1], e_reg=E[2], e_con=E[3])
        self.x = x
        return x[:, :9].astype(f32), x[:, 9:].astype(f32), res


def solve(node_pos, node_t, look, src, t_init, dst, **params):
    """(node_rotations m x 9 f32, node_translations m x 3 f32, result dict) as ssf_graph_solve gives them"""
    return Problem(node_pos, node_t, look, src, t_init, dst, **params).solve()


def deform_points(pts, w4, idx4, node_pos, rot, trans):
    """k_deformation's position formula in f64: sum_n w_n [A_k (p - g_k) + g_k + t_k]"""
    p, g = np.asarray(pts, f64).reshape(-1, 3), np.asarray(node_pos, f64).reshape(-1, 3)
    A, t = np.asarray(rot, f64).reshape(-1, 3, 3), np.asarray(trans, f64).reshape(-1, 3)
    out = np.zeros_like(p)
    for n in range(4):
        k = idx4[:, n]
        out += np.asarray(w4, f64)[:, n, None] * (np.einsum("nij,nj->ni", A[k], p - g[k]) + g[k] + t[k])
    return out


# ---- the independent reference: Gauss-Newton with a sparse direct solve of the normal equations -------------------------------
def direct_gauss_newton(node_pos, edges, w4, idx4, src, dst, w_rot=1.0, w_reg=10.0, w_con=100.0, max_outer=8, outer_tol=1e-6,
                        damping=0.0):
    """the energy of ssf_graph_solve.h minimised by Gauss-Newton, J assembled as a scipy sparse matrix, every step's normal equations
    factorised and solved directly; returns (rotations m x 9 f64, translations m x 3 f64, energies per step)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    g = np.asarray(node_pos, f64).reshape(-1, 3)
    m = len(g)
    s, d, w = np.asarray(src, f64).reshape(-1, 3), np.asarray(dst, f64).reshape(-1, 3), np.asarray(w4, f64)
    nc = len(s)
    sr, sg, sc = np.sqrt(w_rot), np.sqrt(w_reg), np.sqrt(w_con)
    jj, kk = np.repeat(np.arange(m), 4), np.asarray(edges).ravel()
    cc, ck = np.repeat(np.arange(nc), 4), np.asarray(idx4).ravel()
    cw = w.ravel()

    def res_jac(x):
        X = x.reshape(m, 12)
        A, t = X[:, :9].reshape(m, 3, 3), X[:, 9:]
        rows, cols, vals, r = [], [], [], []
        base = 0
        pairs = [(0, 1), (0, 2), (1, 2)]
        for q, (a, b) in enumerate(pairs):                              # column dot products
            r.append(sr * np.einsum("ni,ni->n", A[:, :, a], A[:, :, b]))
            for i in range(3):
                rows += [base + np.arange(m)] * 2
                cols += [12 * np.arange(m) + 3 * i + a, 12 * np.arange(m) + 3 * i + b]
                vals += [sr * A[:, i, b], sr * A[:, i, a]]
            base += m
        for a in range(3):                                              # squared column norms - 1
            r.append(sr * (np.einsum("ni,ni->n", A[:, :, a], A[:, :, a]) - 1))
            for i in range(3):
                rows.append(base + np.arange(m)); cols.append(12 * np.arange(m) + 3 * i + a); vals.append(2 * sr * A[:, i, a])
            base += m
        e = g[kk] - g[jj]
        rr = sg * (np.einsum("nij,nj->ni", A[jj], e) + g[jj] + t[jj] - g[kk] - t[kk])
        ne = len(jj)
        for i in range(3):
            r.append(rr[:, i])
            for c in range(3):
                rows.append(base + np.arange(ne)); cols.append(12 * jj + 3 * i + c); vals.append(sg * e[:, c])
            rows += [base + np.arange(ne)] * 2
            cols += [12 * jj + 9 + i, 12 * kk + 9 + i]
            vals += [np.full(ne, sg), np.full(ne, -sg)]
            base += ne
        u = s[cc] - g[ck]
        vv = cw[:, None] * (np.einsum("nij,nj->ni", A[ck], u) + g[ck] + t[ck] - d[cc])
        for i in range(3):
            r.append(sc * np.bincount(cc, vv[:, i], nc))
            for c in range(3):
                rows.append(base + cc); cols.append(12 * ck + 3 * i + c); vals.append(sc * cw * u[:, c])
            rows.append(base + cc); cols.append(12 * ck + 9 + i); vals.append(sc * cw)
            base += nc
        J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(base, 12 * m))
        return np.concatenate(r), J

    x = np.zeros((m, 12)); x[:, 0] = x[:, 4] = x[:, 8] = 1.0
    x = x.ravel()
    r, J = res_jac(x)
    E = [float(r @ r)]
    for _ in range(max_outer):
        H = (J.T @ J + damping * sp.identity(12 * m)).tocsc()
        x = x + spl.spsolve(H, -(J.T @ r))
        r, J = res_jac(x)
        E.append(float(r @ r))
        if abs(E[-2] - E[-1]) <= outer_tol * E[-2]:
            break
    X = x.reshape(m, 12)
    return X[:, :9].copy(), X[:, 9:].copy(), E
