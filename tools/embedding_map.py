#!/usr/bin/env python3
"""Embedding map of a location encoder: the FastICA colours of its embeddings on a lon/lat grid or at the
locations of a CSV file, on the GPU - the counterpart of the reference's range/evaluation/visualize_embeddings.py.

    python tools/embedding_map.py --location_model_name RANGE+ --pretrained_path satclip-vit16-l40.ckpt \\
        --range_db range_db_large.npz --beta 0.5 --grid 512 1024 --out map_rangeplus
    python tools/embedding_map.py --location_model_name Theory --pretrained_path unused \\
        --input_csv usa_latlon.csv --out map_theory_usa

Writes <out>.npz (``colors`` (N, 3) float64 in [0, 1], ``locs`` (N, 2) lon/lat, ``grid`` (H, W) or empty,
``n_iter``, ``converged``) and <out>.png: ``imshow`` of the (H, W, 3) colours for a grid, a ``scatter`` of the
locations for a CSV.  Unlike the reference's figure there is no map projection and there are no coastlines
(cartopy is not a dependency): the axes are plain longitude and latitude."""
from __future__ import annotations

import argparse
import csv
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def read_lonlat(path: str) -> np.ndarray:
    """(N, 2) float64 (lon, lat) from a CSV with ``lon`` and ``lat`` columns (any other columns are ignored)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows or "lon" not in rows[0] or "lat" not in rows[0]:
        raise SystemExit(f"{path}: needs a header with 'lon' and 'lat' columns")
    return np.array([[float(r["lon"]), float(r["lat"])] for r in rows], dtype=np.float64)


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Embedding map: FastICA colours of a location encoder's embeddings. "
                                "No projection and no coastlines are drawn (no cartopy): plain lon/lat axes.")
    p.add_argument("--location_model_name", type=str, default="RANGE+", help="name of the location model")
    p.add_argument("--pretrained_path", type=str, default="unused",
                   help="SatCLIP / CSP checkpoint (the training-free encoders never read it)")
    p.add_argument("--range_db", type=str, default=None, help="range_db_*.npz bank (RANGE / RANGE+)")
    p.add_argument("--beta", type=float, default=0.5)
    p.add_argument("--input_csv", type=str, default=None, help="CSV with lon and lat columns")
    p.add_argument("--grid", type=int, nargs=2, metavar=("H", "W"), default=None,
                   help="an H x W grid over the globe instead of a CSV")
    p.add_argument("--out", type=str, required=True, help="output path without extension (.npz and .png)")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--seed", type=int, default=2001)
    p.add_argument("--batch_size", type=int, default=100000)
    args = p.parse_args(argv)
    if (args.input_csv is None) == (args.grid is None):
        p.error("give exactly one of --input_csv and --grid H W")
    return args


def main(argv=None) -> int:
    args = get_args(argv)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from range_amd import coord_grid, embedding_map, load_model
    locs = coord_grid(tuple(args.grid)) if args.grid else read_lonlat(args.input_csv)
    kw = {}
    if "RANGE" in args.location_model_name:
        kw = dict(db_path=args.range_db, beta=args.beta)
    model = load_model(args.location_model_name, pretrained_path=args.pretrained_path, device=args.device, **kw)
    colors, info = embedding_map(model, locs, batch_size=args.batch_size, seed=args.seed, return_info=True)
    out = args.out[:-4] if args.out.endswith((".npz", ".png")) else args.out
    np.savez(out + ".npz", colors=colors, locs=np.asarray(locs), grid=np.asarray(args.grid or [], dtype=np.int64),
             n_iter=info["n_iter"], converged=info["converged"])
    rgb = colors if colors.shape[1] == 3 else np.repeat(colors[:, :1], 3, axis=1)
    fig = plt.figure(figsize=(12, 6 if args.grid else 8))
    ax = fig.add_subplot(111)
    if args.grid:
        ax.imshow(rgb.reshape(args.grid[0], args.grid[1], 3), extent=(-180, 180, -90, 90), interpolation="nearest")
    else:
        ax.scatter(locs[:, 0], locs[:, 1], c=rgb, s=1, edgecolor="none")
    ax.set_xlabel("longitude")
    ax.set_ylabel("latitude")
    fig.savefig(out + ".png", bbox_inches="tight", dpi=150)
    plt.close(fig)
    print(f"embedding_map: {len(locs)} locations, {info['n_iter']} FastICA iterations "
          f"({'converged' if info['converged'] else 'NOT converged'}) -> {out}.npz, {out}.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
