"""Backward error of an accepted Levenberg-Marquardt step with respect to the damped normal equations it solves.

CPU only: numpy and the oracle (oracle/), nothing of skeres_amd's native library.  The conventions are oracle/lm.cpp's
(published Ceres):

    solve (J_s^T J_s + D^2) y = J_s^T r,  step = -y,  delta = step * s,  x_k = x_{k-1} (+) delta
    s_j   = 1 / (1 + ||J_j||) of the corrected Jacobian at x0, held for the whole solve (1 without Jacobi scaling)
    D_j^2 = clamp(||J_s,j||^2, min_lm_diagonal, max_lm_diagonal) / radius_{k-1}

From the endpoints x_{k-1} -> x_k of an accepted step the solution the device used is recovered as
y^ = -(x_k - x_{k-1}) / s, and

    eta = ||A y^ - b||_inf / (||A||_inf ||y^||_inf + ||b||_inf),   A = J_s^T J_s + D^2,  b = J_s^T r,

is formed without forming A, every product and sum in long double, from a Jacobian the oracle evaluates in double.  A
backward-stable solve gives eta near the rounding floor whatever the conditioning of A or the elimination order; a wrong
block of the system gives an eta decades above it.  One tolerance TAU therefore covers every plan (check()).

Columns that do not move (constant blocks, coordinates a subset parameterization holds) are dropped: their Jacobian
columns are zeroed, their rows left out of every norm, and they must not have moved at all.
"""
import numpy as np

import oracle

LD = np.longdouble
U_DOUBLE = 2.0 ** -53

# eta <= max(TAU, 4 * floor) for every accepted step.  Observed (profiles/step_backward_error.txt): the oracle's own steps, k = 1..4
# at 6 .. 150 cameras with a loss, constant blocks and a rejected step, <= 1.1e-14 (floors up to 6.7e-14); the device's, every
# plan of tests/test_gpu_step_check.py, <= 8.2e-15; the independent fixture 1.2e-16.  The weakest planted defect of
# tests/test_step_check_cpu.py (S rounded to float32) gives 1.1e-9, the others 2e-7 .. 4e-3.
TAU = 1e-12
CHUNK = 1 << 16


def _require_long_double():
    if np.finfo(LD).nmant < 63:
        raise RuntimeError("step_check needs an 80-bit long double (np.finfo(np.longdouble).nmant = %d)" % np.finfo(LD).nmant)


def log_of(summary):
    """The iteration log of a device summary (list of dicts) or of an oracle Summary, as a list of dicts."""
    if isinstance(summary, list):
        return summary
    if hasattr(summary, "iterations") and callable(summary.iterations):
        return summary.iterations()
    names = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius",
             "step_is_valid", "step_is_successful")
    return [{nm: getattr(summary.iterations[i], nm) for nm in names} for i in range(summary.num_logged)]


def _correct(r, jacs, losses):
    """Ceres' corrector (oracle/loss.hpp loss_correct) on blocks r [nb, k] with Jacobian terms jacs [nb, k, w], in place:
    sqrt(rho') scaling, alpha from rho'', no correction where rho'' <= 0.  losses: None, one spec, or one spec per block."""
    if losses is None:
        return
    nb = r.shape[0]
    if not isinstance(losses, list):
        losses = [losses] * nb
    sq = np.einsum("bk,bk->b", r, r)
    scale_r = np.ones(nb, dtype=LD)
    sqrt_rho1 = np.ones(nb, dtype=LD)
    alpha_sq = np.zeros(nb, dtype=LD)
    for b in range(nb):
        if losses[b] is None or losses[b][0] == "trivial":
            continue
        s = float(sq[b])
        rho = oracle.loss_evaluate(losses[b], s)
        sr1 = np.sqrt(LD(rho[1]))
        sqrt_rho1[b] = sr1
        if s == 0.0 or rho[2] <= 0.0:
            scale_r[b] = sr1
        else:
            alpha = 1 - np.sqrt(1 + 2 * LD(s) * LD(rho[2]) / LD(rho[1]))
            scale_r[b] = sr1 / (1 - alpha)
            alpha_sq[b] = alpha / LD(s)
    for J in jacs:
        rtj = np.einsum("bk,bkw->bw", r, J)
        J -= alpha_sq[:, None, None] * r[:, :, None] * rtj[:, None, :]
        J *= sqrt_rho1[:, None, None]
    r *= scale_r[:, None]


class _Model:
    """A problem as chunks of residual blocks: chunks(x) yields (r [nb, k], [(J [nb, k, w], first column [nb]), ...]), both
    corrected for the loss, long double.  free: bool per column; kind: 0 camera / parameter, 1 eliminated point, 2 retained point."""
    n = 0
    free = None
    kind = None

    def chunks(self, x):
        raise NotImplementedError


class BalModel(_Model):
    """Snavely reprojection blocks of a BalProblem through oracle.bal_evaluate.  loss: None, one spec or a spec per observation;
    cam_mask / pt_mask: bit k = coordinate k held constant (the oracle's convention); retained: indices of retained points."""

    def __init__(self, prob, loss=None, cam_mask=None, pt_mask=None, retained=None):
        self.p = prob
        C, P = prob.num_cameras, prob.num_points
        self.n = 9 * C + 3 * P
        self.loss = loss
        free = np.ones(self.n, dtype=bool)
        if cam_mask is not None:
            free[:9 * C] = ((np.asarray(cam_mask)[:, None] >> np.arange(9)) & 1 == 0).ravel()
        if pt_mask is not None:
            free[9 * C:] = ((np.asarray(pt_mask)[:, None] >> np.arange(3)) & 1 == 0).ravel()
        self.free = free
        self.kind = np.zeros(self.n, dtype=np.int8)
        self.kind[9 * C:] = 1
        if retained is not None:
            for q in np.asarray(retained, dtype=np.int64):
                self.kind[9 * C + 3 * q:9 * C + 3 * q + 3] = 2

    def chunks(self, x):
        p = self.p
        C = p.num_cameras
        r, F, E, _ = oracle.bal_evaluate(C, p.num_points, p.camera_index, p.point_index, p.observations, x)
        fmask = self.free[p.camera_index.astype(np.int64)[:, None] * 9 + np.arange(9)]
        emask = self.free[9 * C + p.point_index.astype(np.int64)[:, None] * 3 + np.arange(3)]
        for a in range(0, p.num_observations, CHUNK):
            sl = slice(a, min(a + CHUNK, p.num_observations))
            rc, Fc, Ec = r[sl].astype(LD), F[sl].astype(LD), E[sl].astype(LD)
            _correct(rc, [Fc, Ec], self.loss[sl] if isinstance(self.loss, list) else self.loss)
            Fc *= fmask[sl][:, None, :]
            Ec *= emask[sl][:, None, :]
            yield rc, [(Fc, 9 * p.camera_index[sl].astype(np.int64)), (Ec, 9 * C + 3 * p.point_index[sl].astype(np.int64))]


class BlocksModel(_Model):
    """General residual blocks through oracle.evaluate: blocks = [(functor id, consts, [parameter block indices], loss or None)];
    parameterizations: None, ("constant",) or ("subset", [held coordinates]) per parameter block."""

    def __init__(self, block_sizes, blocks, parameterizations=None):
        self.sizes = list(block_sizes)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.n = int(self.off[-1])
        self.blocks = blocks
        free = np.ones(self.n, dtype=bool)
        for b, pz in enumerate(parameterizations or [None] * len(self.sizes)):
            if pz is None:
                continue
            held = range(self.sizes[b]) if pz[0] == "constant" else pz[1]
            for c in held:
                free[self.off[b] + c] = False
        self.free = free
        self.kind = np.zeros(self.n, dtype=np.int8)

    def chunks(self, x):
        groups = {}
        for blk in self.blocks:
            groups.setdefault((blk[0], len(blk[2])), []).append(blk)
        for (fid, nbk), members in groups.items():
            rs, Js, losses = [], [[] for _ in range(nbk)], []
            for blk in members:
                params = [x[self.off[i]:self.off[i] + self.sizes[i]] for i in blk[2]]
                ok, res, jac = oracle.evaluate(fid, blk[1], params)
                assert ok
                rs.append(res)
                for t in range(nbk):
                    Js[t].append(jac[t])
                losses.append(blk[3] if len(blk) > 3 else None)
            r = np.array(rs, dtype=LD)
            terms = [np.array(Js[t], dtype=LD) for t in range(nbk)]
            _correct(r, terms, losses)
            out = []
            for t in range(nbk):
                first = np.array([self.off[blk[2][t]] for blk in members], dtype=np.int64)
                cols = first[:, None] + np.arange(terms[t].shape[2])
                terms[t] *= self.free[cols][:, None, :]
                out.append((terms[t], first))
            yield r, out


class DenseRowsModel(_Model):
    """The dense rows of skeres_amd.dense_synth (functor SYNTH_TANH_ROW): r_i = tanh(a_i . x / sqrt(n)) - y_i, one block per
    row over one parameter block of size n, rows in chunks (the Jacobian of the largest cases does not fit in memory twice)."""

    def __init__(self, consts, n, loss=None, chunk=2048):
        from skeres_amd import dense_synth
        self.unit_rows = dense_synth.unit_rows
        self.consts = np.asarray(consts, dtype=np.float64)
        self.n = int(n)
        self.loss = loss
        self.chunk = chunk
        self.free = np.ones(self.n, dtype=bool)
        self.kind = np.zeros(self.n, dtype=np.int8)

    def chunks(self, x):
        n = self.n
        seed = int(self.consts[0, 0])
        inv = 1.0 / np.sqrt(float(n))
        for a in range(0, self.consts.shape[0], self.chunk):
            c = self.consts[a:a + self.chunk]
            A = self.unit_rows(seed, c[:, 1].astype(np.int64), n)
            t = np.tanh((A @ x) * inv)
            r = (t - c[:, 2]).astype(LD)[:, None]
            J = (((1.0 - t * t) * inv)[:, None] * A).astype(LD)[:, None, :]
            _correct(r, [J], self.loss)
            yield r, [(J, np.zeros(len(c), dtype=np.int64))]


class TapeModel(_Model):
    """Residual blocks of recorded functors (skeres_amd/tape.py) evaluated by the long-double interpreter of tests/tape_reference.py
    (run_np; neither device code nor the oracle, which has no tape interpreter).  groups: [(tape, parameter block sizes, captured
    doubles [nb, ncap], offsets [nb, number of blocks] of each block's parameter blocks in x, loss spec or None)]; held: columns
    of x that do not move (constant blocks, coordinates a subset parameterization holds); kind: as _Model's (default 0)."""

    def __init__(self, n, groups, held=(), kind=None, chunk=4096):
        self.n = int(n)
        self.groups = groups
        self.chunk = chunk
        self.free = np.ones(self.n, dtype=bool)
        self.free[np.asarray(list(held), dtype=np.int64)] = False
        self.kind = np.zeros(self.n, dtype=np.int8) if kind is None else np.asarray(kind, dtype=np.int8)

    def chunks(self, x):
        from tape_reference import run_np
        x = np.asarray(x, dtype=np.float64)
        for tape, sizes, captured, offsets, loss in self.groups:
            offsets = np.asarray(offsets, dtype=np.int64)
            captured = np.asarray(captured, dtype=np.float64).reshape(offsets.shape[0], -1)
            for a in range(0, offsets.shape[0], self.chunk):
                o = offsets[a:a + self.chunk]
                X = np.concatenate([x[o[:, q, None] + np.arange(s)] for q, s in enumerate(sizes)], axis=1)
                r, J = run_np(tape, X, captured[a:a + self.chunk], dtype=LD)
                terms, c0 = [], 0
                for s in sizes:
                    terms.append(np.ascontiguousarray(J[:, :, c0:c0 + s]))
                    c0 += s
                _correct(r, terms, loss)
                out = []
                for q, s in enumerate(sizes):
                    terms[q] *= self.free[o[:, q, None] + np.arange(s)][:, None, :]
                    out.append((terms[q], o[:, q]))
                yield r, out


def _scatter(out, first, contrib):
    """out[first[b] + j, :] += contrib[b, j, :] (long double: sort once, np.add.reduceat; np.bincount has no long double)."""
    order = np.argsort(first, kind="stable")
    f = first[order]
    starts = np.flatnonzero(np.r_[True, f[1:] != f[:-1]])
    sums = np.add.reduceat(contrib[order], starts, axis=0)
    w = contrib.shape[1]
    out[f[starts][:, None] + np.arange(w)] += sums


def _column_sq_norms(model, x):
    out = np.zeros((model.n, 1), dtype=LD)
    for r, terms in model.chunks(x):
        for J, first in terms:
            _scatter(out, first, np.einsum("bkw,bkw->bw", J, J)[:, :, None])
    return out[:, 0]


def jacobi_scale(model, x0, jacobi_scaling=True):
    """s_j = 1 / (1 + ||J_j||) of the corrected Jacobian at x0 (1 without Jacobi scaling)."""
    if not jacobi_scaling:
        return np.ones(model.n, dtype=LD)
    return 1 / (1 + np.sqrt(_column_sq_norms(model, x0)))


def backward_error(model, x0, x_prev, x_next, log, k, jacobi_scaling=True, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, scale=None):
    """The backward error of the step x_prev -> x_next, logged as iteration k of `log` (accepted), with respect to the damped
    normal equations at x_prev.  Returns a dict: eta; eta_cameras / eta_points / eta_retained (the same quotient over those
    rows only; NaN where there are none); floor (what the rounding of x_next to doubles alone contributes to eta); mcc and
    mcc_log (model cost change of the helper and cost_change / relative_decrease of the log); gmax and gmax_log (max |J^T r| at
    x_prev, unscaled, and the log's gradient_max_norm of iteration k - 1); moved_fixed (columns held constant that moved); clamped
    (free columns whose ||J_s,j||^2 lies outside [min_lm_diagonal, max_lm_diagonal]: with the default 1e-6 none do on the problems
    of tests/, since ||J_s,j|| = ||J_j|| / (1 + ||J_j||) is far from 0 wherever ||J_j|| is, so a test of the clamp sets
    min_lm_diagonal) and free (columns that may move)."""
    _require_long_double()
    log = log_of(log)
    n = model.n
    x_prev = np.asarray(x_prev, dtype=np.float64)
    x_next = np.asarray(x_next, dtype=np.float64)
    s = jacobi_scale(model, x0, jacobi_scaling) if scale is None else scale
    free = model.free
    z = -(x_next.astype(LD) - x_prev.astype(LD))       # s * y^
    moved_fixed = int(np.count_nonzero(z[~free]))
    z[~free] = 0
    w = U_DOUBLE * np.abs(x_next.astype(LD))            # what rounding x_next may have moved each coordinate by
    w[~free] = 0
    # one pass at x_prev: [col sq norm, J^T r, J^T J z, |J|^T |J| s, |J|^T |J| w]
    acc = np.zeros((n, 5), dtype=LD)
    mcc = LD(0)
    for r, terms in model.chunks(x_prev):
        Jz = np.zeros_like(r)
        As = np.zeros_like(r)
        Aw = np.zeros_like(r)
        cols = []
        for J, first in terms:
            idx = first[:, None] + np.arange(J.shape[2])
            cols.append(idx)
            Ja = np.abs(J)
            Jz += np.einsum("bkw,bw->bk", J, z[idx])
            As += np.einsum("bkw,bw->bk", Ja, s[idx])
            Aw += np.einsum("bkw,bw->bk", Ja, w[idx])
        mcc += np.sum(Jz * (r - Jz / 2))                # -(J_s step).(r + J_s step / 2) with J_s step = -J z
        for (J, first), idx in zip(terms, cols):
            Ja = np.abs(J)
            contrib = np.stack([np.einsum("bkw,bkw->bw", J, J), np.einsum("bkw,bk->bw", J, r), np.einsum("bkw,bk->bw", J, Jz),
                                np.einsum("bkw,bk->bw", Ja, As), np.einsum("bkw,bk->bw", Ja, Aw)], axis=-1)
            _scatter(acc, first, contrib)
    colsq, g, jtjz, aas, aaw = (acc[:, i] for i in range(5))
    radius = LD(log[k - 1]["trust_region_radius"])
    scaled = s * s * colsq
    D2 = np.clip(scaled, LD(min_lm_diagonal), LD(max_lm_diagonal)) / radius
    y = z / s
    Ay = s * jtjz + D2 * y
    b = s * g
    res = np.abs(Ay - b)
    res[~free] = 0
    normA = np.max((s * aas + D2)[free])
    ny = np.max(np.abs(y[free])) if free.any() else LD(0)
    nb = np.max(np.abs(b[free]))
    den = normA * ny + nb
    e = w / s
    floor_res = (s * aaw + D2 * e)
    floor_res[~free] = 0
    out = {"eta": float(np.max(res) / den), "floor": float(np.max(floor_res) / den), "moved_fixed": moved_fixed,
           "clamped": int(np.count_nonzero(((scaled < min_lm_diagonal) | (scaled > max_lm_diagonal)) & free)), "free": int(free.sum())}
    for name, kd in (("eta_cameras", 0), ("eta_points", 1), ("eta_retained", 2)):
        sel = (model.kind == kd) & free
        out[name] = float(np.max(res[sel]) / den) if sel.any() else float("nan")
    out["mcc"] = float(mcc)
    it = log[k]
    out["mcc_log"] = it["cost_change"] / it["relative_decrease"] if it["relative_decrease"] != 0 else float("nan")
    out["gmax"] = float(np.max(np.abs(g)))
    out["gmax_log"] = log[k - 1]["gradient_max_norm"]
    out["y_inf"] = float(ny)
    return out


def check(model, x0, x_prev, x_next, log, k, tol_mcc=1e-10, tol_gmax=1e-11, **kw):
    """backward_error() and its assertions: eta <= max(TAU, 4 floor), the model cost change of the log to tol_mcc relative,
    gradient_max_norm to tol_gmax relative, and no held coordinate moved.  (The floor is a quotient of the normal equations'
    residual, not a bound on the relative error of the model cost change, so it does not widen tol_mcc; observed agreement of
    the model cost change: <= 2e-14 relative.)  Returns the dict."""
    log = log_of(log)
    assert log[k]["step_is_successful"], "iteration %d was not an accepted step" % k
    e = backward_error(model, x0, x_prev, x_next, log, k, **kw)
    assert e["moved_fixed"] == 0, e
    assert e["eta"] <= max(TAU, 4 * e["floor"]), e
    assert abs(e["mcc"] - e["mcc_log"]) <= tol_mcc * abs(e["mcc"]), e
    assert abs(e["gmax"] - e["gmax_log"]) <= tol_gmax * e["gmax"], e
    return e
