"""A numpy restatement of Problem::Evaluate's semantics (include/skeres_amd.h), CPU only: the reference of
tests/test_evaluate_cpu.py and tests/test_gpu_evaluate.py over the cases of tests/evaluate_cases.py.

    raw blocks   oracle.evaluate / oracle.bal_evaluate (double);
    loss         tests/step_check.py's _correct (imported, not copied), long double;
    dPlus        oracle.parameterization_jacobian;
    structure    written here, independently of csrc/evaluate_plan.cpp;
    products and sums in long double.

reference(case) returns a dict: cost, residuals, gradient, rows, cols, values, num_rows, num_cols and what the bounds of compare()
are made of — block_of_value (the residual block, by list position, of every stored entry), block_rows (first row of every listed
block, + end), block_max (each listed block's largest |entry|), grad_scale (per column: sum over the blocks touching it of
||J_b||_max ||r_b||_1) and cost_scale (1/2 sum |rho_b|).

Tolerances of compare(): the project's own device-against-oracle bounds, not this code's figures —
    residuals  rtol 1e-12, atol 1e-9 on the Snavely cases (pixels; tests/test_traced_functors.py) and 1e-12 on unit-scale functors;
    Jacobian   per residual block max |dJ| <= 1e-11 x the block's largest reference entry;
    gradient   per column |dg_j| <= 1e-11 x grad_scale_j;
    cost       1e-11 relative to cost_scale;
    structure  exact.
"""
import numpy as np

import oracle
from step_check import LD, _correct

RTOL_RES, TOL_JAC, TOL_GRAD, TOL_COST = 1e-12, 1e-11, 1e-11, 1e-11


def tangent_size(case, b):
    p = case.parameterizations.get(b)
    return case.sizes[b] if p is None else oracle.parameterization_local_size(p, case.sizes[b])


def _raw(case, ids):
    """Residuals and global-size Jacobians of the listed blocks at case.x, in double: [(r [k], [J_q [k, size_q]])]."""
    out = {}
    snav = [i for i in ids if case.blocks[i][0] == 1 and case.bal_shape is not None]
    if snav:
        C, P = case.bal_shape
        cam = np.array([case.blocks[i][2][0] for i in snav], dtype=np.int32)
        pt = np.array([case.blocks[i][2][1] - C for i in snav], dtype=np.int32)
        obs = np.array([case.blocks[i][1] for i in snav], dtype=np.float64)
        r, F, E, _ = oracle.bal_evaluate(C, P, cam, pt, obs, case.x)
        for k, i in enumerate(snav):
            out[i] = (r[k], [F[k], E[k]])
    for i in ids:
        if i in out:
            continue
        fid, consts, pbs = case.blocks[i][:3]
        ok, r, jac = oracle.evaluate(fid, consts, [case.x[case.off[b]:case.off[b] + case.sizes[b]] for b in pbs])
        assert ok
        out[i] = (r, jac)
    return out


def reference(case, structure_only=False, defect=None):
    """defect (tests of compare() itself): "no_loss" — the loss correction left out of the values; "no_projection" — the first
    tangent-size columns of the global Jacobian instead of J * dPlus for quaternion / homogeneous blocks."""
    columns = case.parameter_blocks if case.parameter_blocks is not None else case.first_seen()
    col_off, n = {}, 0
    for b in columns:
        col_off[b] = n
        n += tangent_size(case, b)
    ids = list(case.residual_blocks) if case.residual_blocks is not None else list(range(len(case.blocks)))
    # structure: rows in list order; per row the stored blocks in ascending column order
    rows, cols, block_rows, slots_of = [0], [], [0], []
    for i in ids:
        fid, consts, pbs = case.blocks[i][:3]
        nres = oracle.functor_info(fid)[0]
        stored = sorted((col_off[b], q, b) for q, b in enumerate(pbs) if b in col_off and b not in case.constant and tangent_size(case, b) > 0)
        slots_of.append(stored)
        row_cols = [c0 + j for c0, q, b in stored for j in range(tangent_size(case, b))]
        for _ in range(nres):
            cols.extend(row_cols)
            rows.append(len(cols))
        block_rows.append(block_rows[-1] + nres)
    out = {"num_rows": block_rows[-1], "num_cols": n, "rows": np.array(rows, dtype=np.int64), "cols": np.array(cols, dtype=np.int64),
           "block_rows": np.array(block_rows, dtype=np.int64)}
    if structure_only:
        return out

    raw = _raw(case, ids)
    dplus = {}
    for b, p in case.parameterizations.items():
        dplus[b] = oracle.parameterization_jacobian(p, case.x[case.off[b]:case.off[b] + case.sizes[b]]).astype(LD)
    residuals = np.zeros(out["num_rows"], dtype=LD)
    values = np.zeros(len(cols), dtype=LD)
    gradient = np.zeros(n, dtype=LD)
    grad_scale = np.zeros(n, dtype=LD)
    block_of_value = np.zeros(len(cols), dtype=np.int64)
    block_max = np.zeros(len(ids), dtype=LD)
    cost = cost_scale = LD(0)
    for k, i in enumerate(ids):
        loss = case.blocks[i][3] if case.apply_loss else None
        r0, jac0 = raw[i]
        s = float(np.dot(r0, r0))
        rho0 = oracle.loss_evaluate(loss, s)[0] if loss is not None else s
        cost += LD(rho0) / 2
        cost_scale += abs(LD(rho0)) / 2
        r = np.array(r0, dtype=LD)[None, :]
        jacs = [np.array(j, dtype=LD)[None, :, :] for j in jac0]
        if defect == "no_loss":
            rr = r.copy()
            _correct(rr, [], loss)       # the residuals corrected, the Jacobian not
            r = rr
        else:
            _correct(r, jacs, loss)
        r = r[0]
        residuals[block_rows[k]:block_rows[k + 1]] = r
        nres = len(r)
        parts = []
        for c0, q, b in slots_of[k]:
            J = jacs[q][0]
            if b in dplus:
                J = J[:, :dplus[b].shape[1]] if (defect == "no_projection" and case.parameterizations[b][0] in ("quaternion", "homogeneous")) else J @ dplus[b]
            parts.append((c0, J))
        if not parts:
            continue
        block = np.concatenate([J for _, J in parts], axis=1)
        first = rows[block_rows[k]]
        values[first:first + block.size] = block.ravel()
        block_of_value[first:first + block.size] = k
        block_max[k] = np.max(np.abs(block))
        r1 = np.sum(np.abs(r))
        for c0, J in parts:
            gradient[c0:c0 + J.shape[1]] += r @ J
            grad_scale[c0:c0 + J.shape[1]] += block_max[k] * r1
    out.update({"cost": cost, "cost_scale": cost_scale, "residuals": residuals, "values": values, "gradient": gradient, "grad_scale": grad_scale,
                "block_of_value": block_of_value, "block_max": block_max})
    return out


def compare(ref, got, case):
    """got: dict with any of cost, residuals, gradient, rows, cols, values.  Returns the largest ratio to each bound that was checked
    ({"residuals": ..., "jacobian": ..., "gradient": ..., "cost": ...}); the structure must be equal.  A ratio above 1 is a failure:
    check() asserts."""
    ratios = {}
    if "rows" in got:
        assert np.array_equal(np.asarray(got["rows"], dtype=np.int64), ref["rows"]), "rows differ"
        assert np.array_equal(np.asarray(got["cols"], dtype=np.int64), ref["cols"]), "cols differ"
    if "residuals" in got:
        atol = 1e-9 if case.snavely else 1e-12
        d = np.abs(np.asarray(got["residuals"], dtype=LD) - ref["residuals"])
        ratios["residuals"] = float(np.max(d / (atol + RTOL_RES * np.abs(ref["residuals"])))) if len(d) else 0.0
    if "values" in got:
        d = np.abs(np.asarray(got["values"], dtype=LD) - ref["values"])
        assert d.shape == ref["values"].shape, "number of stored entries differs"
        per_block = np.zeros(len(ref["block_max"]), dtype=LD)
        np.maximum.at(per_block, ref["block_of_value"], d)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(ref["block_max"] > 0, per_block / (TOL_JAC * ref["block_max"]), np.where(per_block > 0, np.inf, 0))
        ratios["jacobian"] = float(np.max(q)) if len(q) else 0.0
    if "gradient" in got:
        d = np.abs(np.asarray(got["gradient"], dtype=LD) - ref["gradient"])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(ref["grad_scale"] > 0, d / (TOL_GRAD * ref["grad_scale"]), np.where(d > 0, np.inf, 0))
        ratios["gradient"] = float(np.max(q)) if len(q) else 0.0
    if "cost" in got:
        ratios["cost"] = float(abs(LD(got["cost"]) - ref["cost"]) / (TOL_COST * ref["cost_scale"]))
    return ratios


def check(ref, got, case):
    ratios = compare(ref, got, case)
    for name, q in ratios.items():
        assert q <= 1.0, "%s: %s is %.3g times its bound" % (case.name, name, q)
    return ratios


_REFERENCES = {}


def reference_of(name):
    """The reference of a case of evaluate_cases.CASES: computed once, shared, left unchanged."""
    import evaluate_cases
    if name not in _REFERENCES:
        _REFERENCES[name] = reference(evaluate_cases.case(name))
    return _REFERENCES[name]
