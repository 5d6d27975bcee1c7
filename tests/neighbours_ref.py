"""Comparator of d3p_pair_knn and d3p_amd.neighbours in numpy: the float32 chain of tests/fidelity_ref.py, the k nearest as
the first k of a sort by (q, j), the counts by the strict rule, prdc by the module docstring's formulas.  Nothing reaches a device."""
import numpy as np

from tests.fidelity_ref import _admissible, _as2, _bad_rows, _q32


def knn(a, b, k, exclude_diagonal=False, radius_sq=None):
    a, b = _as2(a), _as2(b)
    na, nb = a.shape[0], b.shape[0]
    with np.errstate(all="ignore"):
        q = _q32(a[:, None, :], b[None, :, :])
    ok, bad = _admissible(na, nb, exclude_diagonal), _bad_rows(a, b)
    out = {"sq": np.full((na, k), np.inf, np.float32), "index": np.full((na, k), -1, np.int64)}
    for i in range(na):
        js = np.nonzero(ok[i])[0]
        js = js[np.lexsort((js, q[i, js]))][:k]            # by q, then by j
        out["sq"][i, :js.size], out["index"][i, :js.size] = q[i, js], js
    out["sq"][bad], out["index"][bad] = np.nan, -1
    with np.errstate(all="ignore"):
        out["distance"] = np.sqrt(out["sq"]).astype(np.float32)
        if radius_sq is not None:
            out["count"] = np.where(bad, -1, (ok & (q < np.asarray(radius_sq, np.float32)[None, :])).sum(axis=1)).astype(np.int64)
    return out


def prdc(real, synthetic, k, holdout=None):
    R, S = _as2(real), _as2(synthetic)
    rr, ss = knn(R, R, k, True), knn(S, S, k, True)
    sr, rs = knn(S, R, 1, radius_sq=rr["sq"][:, k - 1]), knn(R, S, 1, radius_sq=ss["sq"][:, k - 1])
    return {"precision": float((sr["count"] > 0).mean()), "recall": float((rs["count"] > 0).mean()),
            "density": float(sr["count"].sum()) / (k * S.shape[0]), "coverage": float((rs["sq"][:, 0] < rr["sq"][:, k - 1]).mean()),
            "authenticity": float((sr["sq"][:, 0] > rr["sq"][sr["index"][:, 0], 0]).mean()),
            "floor": prdc(real, holdout, k) if holdout is not None else None}
