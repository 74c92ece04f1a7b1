"""Float64 yardstick, per-frame gate and float32 restatement of the shared-intrinsics LM step (shared_step_kernel /
gclm_shared_reduce + gclm_shared_apply in geocalib_amd/csrc/gclm_update.hip), shared by the CPU self-check
(test_shared_gate.py) and the GPU parity test (test_shared_step_parity.py).

Reference: one float64 step of the oracle's dense arrow-head solve (lm_optimizer.py:350-383) per group, from the kernel's
own state (test_step_parity._oracle_step).  Gate: test_step_oracle.step_gate per frame, with tau scaled by the group's own
conditioning.  Scaled by its diagonal, the group's damped float64 system has its eigenvalues in [lambda, rho_g + lambda],
rho_g the spectral radius of the undamped scaled (2N + ni)^2 system; the existing gate rests on the per-image bound
kappa_P = (P + lambda) / lambda (P = 2 + ni: a one-image system has trace P), so a group is allowed
    tau * max(1, kappa_g / kappa_P),   kappa_g = (rho_g + lambda) / lambda,
which is exactly tau for a one-frame group (rho_g <= trace = P).  Measured: kappa_g stays below kappa_P for every group
of the tests (up to 2048 frames), so the scale is 1 there.

Restatement: the kernel's Schur step in float32, in its order, from float32 per-frame systems -- the frame's damped 2x2
gravity block and its contribution (E^T D^-1 E, E^T D^-1 g, H_II, g_I); their float32 group sum in frame order; damping
max(sum H_ii lambda, 1e-6) on the summed intrinsic diagonal; the NI x NI Cholesky; the 2x2 back-substitution per frame;
the update (log focal, distortion clamp, spherical gravity).  `mutant` names one plausible kernel bug each, for the
gate-power tests."""
import numpy as np

from test_step_oracle import TAU_FLOOR, TAU_REL, div_k_allowance, step_gate

NI = {"pinhole": 1, "simple_radial": 2, "radial": 3, "simple_divisional": 2}
TILE = 64                   # kTileFrames: frames per reduction tile of shared_step_kernel
APPLY_STRIDE = 256          # kGroups * kSlots: the one-call apply loop's stride
F32 = np.float32
MUTANTS = ("drop_after_tile1", "last_tile_twice", "apply_first_256", "lower_bound_off_by_one", "damp_S", "no_EDg",
           "radial_k2_dropped", "S_transposed")


def groups_of(gof):
    """Frame index arrays of each group from a sorted group_of_frame (groups absent from it are empty)."""
    gof = np.asarray(gof)
    G = int(gof.max()) + 1 if len(gof) else 0
    return [np.arange(lo, hi) for lo, hi in zip(np.searchsorted(gof, np.arange(G), "left"),
                                                 np.searchsorted(gof, np.arange(G), "right"))]


def oracle_conf(model):
    return {"camera_model": model, "shared_intrinsics": True, "fix_lambda": True}


def reference_step(oracle, model, data, start, lam, groups, precision="f64"):
    """One dense arrow-head step of every group from `start` = (cam, grav) (test_step_parity._oracle_step, one call per
    group); returns camera, gravity and step_failures of the whole batch."""
    from test_step_parity import _oracle_step
    cam, grav = start
    B = len(cam)
    out = {"camera": cam.copy(), "gravity": grav.copy(), "step_failures": np.zeros(B, np.float32)}
    for idx in groups:
        if len(idx) == 0:
            continue
        part = {k: (v[idx] if k != "scales" else v) for k, v in data.items()}
        r = _oracle_step(oracle, {**oracle_conf(model), "group_size": None}, part, (cam[idx], grav[idx]), lam[idx],
                         precision)
        for k in out:
            out[k][idx] = r[k]
    return out


def frame_systems(oracle, model, data, cam, grav, precision="f64"):
    """Per-frame (H (B, P, P), G (B, P)) at (cam, grav), P = 2 + ni."""
    s = oracle.system(data, cam, grav, oracle_conf(model), precision=precision)
    return s["H"], s["G"]


def group_scale(model, H, lam, groups):
    """Per frame (B,): max(1, kappa_g / kappa_P) of its group and kappa_g, from the float64 per-frame systems H (B, P, P)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.linalg import eigsh
    ni = NI[model]
    P = 2 + ni
    lam = float(lam)
    scale, kappa = np.ones(len(H)), np.zeros(len(H))
    for idx in groups:
        N = len(idx)
        if N == 0:
            continue
        Hg = np.asarray(H[idx], np.float64)
        n = 2 * N + ni
        rows, cols, vals = [], [], []
        fr = 2 * np.arange(N)
        for i in range(2):
            for j in range(2):
                rows.append(fr + i); cols.append(fr + j); vals.append(Hg[:, i, j])
            for j in range(ni):
                rows += [fr + i, np.full(N, 2 * N + j)]
                cols += [np.full(N, 2 * N + j), fr + i]
                vals += [Hg[:, i, 2 + j], Hg[:, 2 + j, i]]
        Cs = Hg[:, 2:, 2:].sum(0)
        ii, jj = np.meshgrid(np.arange(ni), np.arange(ni), indexing="ij")
        rows.append(2 * N + ii.ravel()); cols.append(2 * N + jj.ravel()); vals.append(Cs.ravel())
        A = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
        d = 1 / np.sqrt(A.diagonal())
        A = A.multiply(d[:, None]).multiply(d[None, :]).tocsr()
        if n <= 512:
            rho = np.linalg.eigvalsh(A.toarray())[-1]
        else:
            rho = eigsh(A, k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0]
        rho = min(rho, n)                      # the trace: exact bound (and rho <= P for one frame)
        kg, kP = (rho + lam) / lam, (P + lam) / lam
        scale[idx], kappa[idx] = max(1.0, kg / kP), kg
    return scale, kappa


def gate_terms(oracle, model, data, start, lam, groups):
    """What the gate of a step from `start` needs: the float64 reference step ("ref64"), the per-frame scale and kappa_g
    of its group ("scale", "kappa"), simple_divisional's k allowance ("extra": test_step_oracle.div_k_allowance; its
    first step only is gated, DIV_STEPS)."""
    ref64 = reference_step(oracle, model, data, start, lam, groups)
    H, _ = frame_systems(oracle, model, data, *start)
    scale, kappa = group_scale(model, H, lam[0], groups)
    extra = None
    if model == "simple_divisional":
        extra = div_k_allowance(model, reference_step(oracle, model, data, start, lam, groups, "f32"), ref64)
    return {"ref64": ref64, "scale": scale, "kappa": kappa, "extra": extra}


def gate(start, got, model, terms):
    """Ratio (B, components) of a step `got` = (cam, grav) from `start` to the float64 gate; <= 1 passes."""
    ref, scale = terms["ref64"], terms["scale"][:, None]
    return step_gate(model, start, got, (ref["camera"], ref["gravity"]), TAU_REL * scale, TAU_FLOOR * scale,
                     terms["extra"])


# ------------------------------------------------------------------ the float32 restatement

def _frame_terms(H, G, lam, ni):
    """Per frame, float32: Dinv (B, 2, 2), ok (B,), and the contribution (B, 24) in the partial layout
    [0..9) E^T Dinv E (3x3, row j col i = E_j . Dinv E_i), [9..12) E^T Dinv g, [12..21) H_II, [21..24) g_I."""
    B = len(H)
    one_m6 = F32(1e-6)
    a = H[:, 0, 0] + np.maximum(H[:, 0, 0] * lam, one_m6)
    b = H[:, 0, 1]
    d = H[:, 1, 1] + np.maximum(H[:, 1, 1] * lam, one_m6)
    det = a * d - b * b
    with np.errstate(all="ignore"):
        idt = F32(1) / det
    ok = (a > 0) & (det > 0)
    Dinv = np.stack([np.stack([d * idt, -b * idt], -1), np.stack([-b * idt, a * idt], -1)], -2)
    q0 = Dinv[:, 0, 0] * G[:, 0] + Dinv[:, 0, 1] * G[:, 1]
    q1 = Dinv[:, 1, 0] * G[:, 0] + Dinv[:, 1, 1] * G[:, 1]
    o = np.zeros((B, 24), F32)
    for i in range(ni):
        e0, e1 = H[:, 0, 2 + i], H[:, 1, 2 + i]
        t0 = Dinv[:, 0, 0] * e0 + Dinv[:, 0, 1] * e1
        t1 = Dinv[:, 1, 0] * e0 + Dinv[:, 1, 1] * e1
        for j in range(ni):
            o[:, j * 3 + i] = H[:, 0, 2 + j] * t0 + H[:, 1, 2 + j] * t1
            o[:, 12 + i * 3 + j] = H[:, 2 + i, 2 + j]
        o[:, 9 + i] = e0 * q0 + e1 * q1
        o[:, 21 + i] = G[:, 2 + i]
    return Dinv, ok, o


def _group_sum(o):
    """Sum of the contributions (N, 24) over the frames of a group: float32, in frame order (the kernel's step (3): the
    tiles follow each other, so the tile split does not change the order)."""
    if len(o) == 0:
        return np.zeros(24, F32)
    return np.cumsum(o, axis=0, dtype=F32)[-1]


def _chol_solve(A, b):
    """chol_solve<N> of gclm_device.h in float32 (scalar loop, its order)."""
    n = len(b)
    A, b = A.astype(F32).copy(), b.astype(F32).copy()
    ok = True
    with np.errstate(all="ignore"):
        for j in range(n):
            s = A[j, j]
            for k in range(j):
                s = F32(s - A[j, k] * A[j, k])
            ok = ok and bool(s > 0)
            l = F32(np.sqrt(s))
            A[j, j] = l
            for i in range(j + 1, n):
                t = A[i, j]
                for k in range(j):
                    t = F32(t - A[i, k] * A[j, k])
                A[i, j] = F32(t / l)
        for i in range(n):
            t = b[i]
            for k in range(i):
                t = F32(t - A[i, k] * b[k])
            b[i] = F32(t / A[i, i])
        for i in range(n - 1, -1, -1):
            t = b[i]
            for k in range(i + 1, n):
                t = F32(t - A[k, i] * b[k])
            b[i] = F32(t / A[i, i])
    return b, ok


def _grav_update(g, d0, d1):
    """Spherical Gravity.update (gclm_device.h grav_update_pre / _post), float32, per row."""
    g = g.astype(F32)
    x, y, z = g[:, 0], g[:, 1], g[:, 2]
    with np.errstate(all="ignore"):
        nx = np.sqrt(x * x + y * y + z * z)
        sigma = x * x + y * y
        norm = np.sqrt(sigma + z * z)
        sigma = np.where(sigma < F32(1e-7), sigma + F32(1e-7), sigma)
        vpiv = np.where(z < 0, z - norm, -sigma / (z + norm))
        beta = F32(2) * vpiv * vpiv / (sigma + vpiv * vpiv)
        v = [x / vpiv, y / vpiv, np.ones_like(x)]
        nd = np.sqrt(d0 * d0 + d1 * d1)
        eps = F32(1e-7)
        nd_ = np.where(nd < eps, nd + eps, nd)
        sinc = np.where(nd < eps, F32(1), np.sin(nd_) / nd_)
        e = [sinc * d0, sinc * d1, np.cos(nd)]
        bd = beta * (v[0] * e[0] + v[1] * e[1] + v[2] * e[2])
        out = np.stack([nx * (e[k] - v[k] * bd) for k in range(3)], -1)
        n = np.maximum(np.sqrt((out * out).sum(-1, dtype=F32)), F32(1e-12))
    return (out / n[:, None]).astype(F32)


def restate_step(model, H, G, cam, grav, lam, groups, mutant=None):
    """The shared step of every group from float32 per-frame systems H (B, P, P), G (B, P) at state (cam, grav), lambda
    `lam` (B,); returns (camera, gravity, failed (B,) bool)."""
    assert mutant is None or mutant in MUTANTS, mutant
    ni = NI[model]
    H, G = np.asarray(H, F32), np.asarray(G, F32)
    cam, grav = np.asarray(cam, F32).copy(), np.asarray(grav, F32).copy()
    lam = np.asarray(lam, F32)
    B = len(cam)
    Dinv, ok_f, o = _frame_terms(H, G, lam, ni)
    if mutant == "S_transposed":               # kGS filled as [i][j] = E_i . Dinv E_j instead of [j][i]
        o = o.copy()
        S = o[:, :9].reshape(B, 3, 3)
        o[:, :9] = S.transpose(0, 2, 1).reshape(B, 9)
    if mutant == "lower_bound_off_by_one":     # both ends of every group's range one frame late: [f0 + 1, f1 + 1)
        groups = [np.arange(min(g[0] + 1, B), min(g[-1] + 2, B)) if len(g) else g for g in groups]
    dI = np.zeros((B, 3), F32)
    dG = np.zeros((B, 2), F32)
    failed = np.zeros(B, bool)
    applied = np.zeros(B, bool)
    one_m6 = F32(1e-6)
    for idx in groups:
        if len(idx) == 0:
            continue
        og = o[idx]
        if mutant == "drop_after_tile1":
            og = og[:TILE]
        elif mutant == "last_tile_twice":
            last = (len(idx) - 1) // TILE * TILE
            og = np.concatenate([og, og[last:]])
        s = _group_sum(og)
        ok = bool(ok_f[idx].all())
        lg = lam[idx[0]]
        A = np.zeros((ni, ni), F32)
        rhs = np.zeros(ni, F32)
        for i in range(ni):
            rhs[i] = s[21 + i] if mutant == "no_EDg" else F32(s[21 + i] - s[9 + i])
            for j in range(ni):
                Sij = s[i * 3 + j]
                if mutant == "radial_k2_dropped" and ni == 3 and 2 in (i, j):
                    Sij = F32(0)
                A[i, j] = F32(s[12 + i * 3 + j] - Sij)
            if mutant == "damp_S":
                A[i, i] = F32(A[i, i] + max(F32(A[i, i] * lg), one_m6))
            else:
                A[i, i] = F32(A[i, i] + max(F32(s[12 + i * 3 + i] * lg), one_m6))
        x, cok = _chol_solve(A, rhs)
        ok = ok and cok and bool(np.all(np.abs(x) <= F32(3.0e38)))
        upd = idx[:APPLY_STRIDE] if mutant == "apply_first_256" else idx
        applied[upd] = True
        if not ok:
            failed[upd] = True
            continue
        dI[upd, :ni] = x
        r0, r1 = G[upd, 0].copy(), G[upd, 1].copy()
        for i in range(ni):
            r0 = r0 - H[upd, 0, 2 + i] * x[i]
            r1 = r1 - H[upd, 1, 2 + i] * x[i]
        g0 = Dinv[upd, 0, 0] * r0 + Dinv[upd, 0, 1] * r1
        g1 = Dinv[upd, 1, 0] * r0 + Dinv[upd, 1, 1] * r1
        bad = ~((np.abs(g0) <= F32(3e38)) & (np.abs(g1) <= F32(3e38)))
        failed[upd] |= bad
        dG[upd] = np.stack([np.where(bad, F32(0), g0), np.where(bad, F32(0), g1)], -1)
    # the update (frames no group applies to keep their state)
    new_grav = _grav_update(grav, dG[:, 0], dG[:, 1])
    grav = np.where(applied[:, None], new_grav, grav)
    h, fx, fy = cam[:, 1], cam[:, 2], cam[:, 3]
    with np.errstate(all="ignore"):
        nfy = np.exp(np.log(fy) + dI[:, 0])
        min_f, max_f = h * F32(0.5) / F32(3.7320504), h * F32(0.5) / F32(0.043660942)
        fyc = np.minimum(np.maximum(nfy, min_f), max_f)
        nfx = fyc * fx / fy
    cam[:, 2] = np.where(applied, nfx, fx)
    cam[:, 3] = np.where(applied, fyc, fy)
    if ni >= 2:
        hi = F32(3.0) if model == "simple_divisional" else F32(0.7)
        k1 = np.clip(cam[:, 6] + dI[:, 1], -hi, hi)
        k2 = np.clip(cam[:, 7] + (dI[:, 2] if model == "radial" else dI[:, 1]), -hi, hi)
        cam[:, 6] = np.where(applied, k1, cam[:, 6])
        cam[:, 7] = np.where(applied, k2, cam[:, 7])
    return cam, grav, failed
