#!/usr/bin/env python3
"""Golden vectors of the embedding map (range_amd/embedding_map.py), generated on the CPU in the development
container with the installed scikit-learn (never on the GPU box):

    python tests/golden/make_golden_icamap.py

``icamap.npz`` holds, per fixture F (inputs are float32 so that the file stays small; every consumer widens them
to float64 first, exactly):

* ``F_X`` the features; ``synth_600x50`` / ``synth_601x130``: independent uniform / Laplace / bimodal /
  exponential sources mixed by a Gaussian matrix plus 0.05 noise (tests/icamap_refs.py: synth_features);
  ``sphere_640x96``: sin(P W + b) of the unit vectors P of ``coord_grid((20, 32))`` with column 7 set to the
  constant 0.25 (the reference's 1e-8 rule, visualize_embeddings.py:123);
* per run R of that fixture (``c3`` everywhere; for the sphere also ``c2``, ``c5`` when it meets the conditions
  below, and ``c3_it3`` = max_iter 3): ``F_R_svd`` / ``F_R_eigh`` the sources
  ``FastICA(n_components=c, random_state=2001, whiten='unit-variance', max_iter=1000, whiten_solver=...)
  .fit(Xs).transform(Xs)`` of the standardised matrix Xs (visualize_embeddings.py:121-135), ``F_R_n_iter``,
  ``F_R_limits`` (the convergence limit of every iteration, from the numpy restatement of ``_ica_par`` in
  tests/icamap_refs.py) and ``F_R_d_ref`` = max |svd - eigh|;
* ``grid_5x7`` / ``grid_4x6_split``: what the reference's own ``coord_grid`` (its function object is compiled
  from the reference file at generation time, nothing of it is copied) returns for (5, 7), and for (4, 6) with
  a split mask ``grid_split_ids`` and split 2.

Conditions asserted on every run (on the fixtures, not measurements): scikit-learn converges (except ``it3``), both
solvers stop at the same iteration, every limit is at least 1 % of tol away from tol, the first entry of each
kept eigenvector exceeds 1e-3, the kept eigenvalues are 5 % apart from each other and from the next one."""
from __future__ import annotations

import ast
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import icamap_refs as R  # noqa: E402
import make_golden as mg  # noqa: E402

SEED = 2001


def reference_coord_grid():
    path = os.path.join(mg.REF, "range", "evaluation", "visualize_embeddings.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "coord_grid"]
    ns = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["coord_grid"]


def sphere_features(coord_grid):
    locs = coord_grid((20, 32)).astype(np.float64)
    lon, lat = np.radians(locs[:, 0]), np.radians(locs[:, 1])
    P = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1)
    rng = np.random.default_rng(77)
    X = np.sin(np.dot(P, 2.0 * rng.standard_normal((3, 96))) + rng.uniform(0, 2 * np.pi, 96))
    X[:, 7] = 0.25
    return X


def conditions_hold(X, c, limits, tol=R.TOL):
    Xs = R.standardise(X)[0]
    lam, u, nxt = R.eig_top(Xs, c)
    ok = bool(np.all(np.abs(u[0]) > 1e-3))
    seq = np.append(lam, nxt)
    ok &= bool(np.all(seq[:-1] - seq[1:] >= 0.05 * seq[:-1]))
    ok &= bool(np.all(np.abs(limits - tol) >= 0.01 * tol))
    return ok


def run(X, c, max_iter=1000):
    from sklearn.decomposition import FastICA
    from sklearn.exceptions import ConvergenceWarning
    Xs = R.standardise(X)[0]
    out = {}
    for solver in ("svd", "eigh"):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ica = FastICA(n_components=c, random_state=SEED, whiten="unit-variance", max_iter=max_iter,
                          whiten_solver=solver)
            ica.fit(Xs)
            out[solver] = ica.transform(Xs)
        out[solver + "_n_iter"] = ica.n_iter_
        out[solver + "_converged"] = not any(issubclass(x.category, ConvergenceWarning) for x in w)
    ref = R.fastica_sources(X, c, SEED, max_iter)
    out["limits"] = ref["limits"]
    out["restated"] = float(np.abs(ref["sources"] - out["svd"]).max())
    out["d_ref"] = float(np.abs(out["svd"] - out["eigh"]).max())
    return out


def main():
    coord_grid = reference_coord_grid()
    fixtures = {"synth_600x50": R.synth_features(600, 50, 11), "synth_601x130": R.synth_features(601, 130, 12),
                "sphere_640x96": sphere_features(coord_grid)}
    gold = {}
    for name, X in fixtures.items():
        X = X.astype(np.float32)
        gold[name + "_X"] = X
        X = X.astype(np.float64)
        runs = [("c3", 3, 1000)]
        if name.startswith("sphere"):
            runs += [("c2", 2, 1000), ("c5", 5, 1000), ("c3_it3", 3, 3)]
        for tag, c, max_iter in runs:
            r = run(X, c, max_iter)
            ok = conditions_hold(X, c, r["limits"]) and r["svd_n_iter"] == r["eigh_n_iter"] == len(r["limits"])
            ok &= (r["svd_converged"] and r["eigh_converged"]) == (max_iter == 1000)
            print(f"{name} {tag}: n_iter {r['svd_n_iter']} d_ref {r['d_ref']:.2e} restated-svd {r['restated']:.2e} "
                  f"last limit {r['limits'][-1]:.3e} conditions {'hold' if ok else 'FAIL'}")
            if not ok and tag == "c5":
                continue                        # (optional run: kept only when it meets the conditions)
            assert ok, (name, tag)
            key = f"{name}_{tag}_"
            gold[key + "svd"], gold[key + "eigh"] = r["svd"], r["eigh"]
            gold[key + "n_iter"], gold[key + "limits"], gold[key + "d_ref"] = r["svd_n_iter"], r["limits"], r["d_ref"]
    gold["grid_5x7"] = coord_grid((5, 7))
    ids = np.arange(24).reshape(4, 6) % 3
    gold["grid_split_ids"] = ids
    gold["grid_4x6_split"] = coord_grid((4, 6), ids, 2)
    path = os.path.join(HERE, "icamap.npz")
    np.savez(path, **gold)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
