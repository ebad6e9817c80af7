#!/usr/bin/env python3
"""Cluster map of a location encoder: the complete-linkage cosine clusters of its embeddings on a lon/lat grid or at
the locations of a CSV file, on the GPU - the counterpart of the reference's spa_enc_embed_clustering and make_enc_map
(location_models/csp/main/analysis.py:386-475).

    python tools/cluster_map.py --location_model_name RANGE+ --pretrained_path satclip-vit16-l40.ckpt \\
        --range_db range_db_large.npz --beta 0.5 --grid 180 360 --n_clusters 30 --out clusters_rangeplus
    python tools/cluster_map.py --location_model_name Theory --input_csv usa_latlon.csv --n_clusters 12 \\
        --out clusters_theory_usa

Writes <out>.npz (``labels`` (H, W) or (N,) int32 numbered by first occurrence, ``locs`` (N, 2) lon/lat, ``grid``
(H, W) or empty, ``n_clusters``, ``linkage`` scipy's Z, ``rounds``) and <out>.png: ``imshow`` of the labels for a
grid, a ``scatter`` of the locations for a CSV, in the reference's ``terrain`` colours.  Unlike the reference's figure
there are no coastlines and no mask outlines (its shapefile overlays are not a dependency): the axes are plain
longitude and latitude.  ``--mask_npy`` is the reference's land mask: an array with one value per location, 0 = ocean;
the masked cells all land in one cluster."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.embedding_map import read_lonlat  # noqa: E402


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Cluster map: complete-linkage cosine clusters of a location encoder's "
                                "embeddings.  There are no coastlines and no mask outlines: plain lon/lat axes.")
    p.add_argument("--location_model_name", type=str, default="RANGE+", help="name of the location model")
    p.add_argument("--pretrained_path", type=str, default="unused",
                   help="SatCLIP / CSP checkpoint (the training-free encoders never read it)")
    p.add_argument("--range_db", type=str, default=None, help="range_db_*.npz bank (RANGE / RANGE+)")
    p.add_argument("--beta", type=float, default=0.5)
    p.add_argument("--input_csv", type=str, default=None, help="CSV with lon and lat columns")
    p.add_argument("--grid", type=int, nargs=2, metavar=("H", "W"), default=None,
                   help="an H x W grid over the globe instead of a CSV")
    p.add_argument("--n_clusters", type=int, required=True)
    p.add_argument("--mask_npy", type=str, default=None, help=".npy with one value per location, 0 = masked (ocean)")
    p.add_argument("--out", type=str, required=True, help="output path without extension (.npz and .png)")
    p.add_argument("--device", type=str, default="cuda")
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

    from range_amd import cluster_map, coord_grid, load_model
    locs = coord_grid(tuple(args.grid)) if args.grid else read_lonlat(args.input_csv)
    mask = np.load(args.mask_npy) if args.mask_npy else None
    kw = {}
    if "RANGE" in args.location_model_name:
        kw = dict(db_path=args.range_db, beta=args.beta)
    model = load_model(args.location_model_name, pretrained_path=args.pretrained_path, device=args.device, **kw)
    labels, info = cluster_map(model, locs, args.n_clusters, grid_size=args.grid, mask=mask,
                               batch_size=args.batch_size, return_info=True)
    out = args.out[:-4] if args.out.endswith((".npz", ".png")) else args.out
    np.savez(out + ".npz", labels=labels, locs=np.asarray(locs), grid=np.asarray(args.grid or [], dtype=np.int64),
             n_clusters=args.n_clusters, linkage=info["linkage"], rounds=info["rounds"])
    fig = plt.figure(figsize=(12, 6 if args.grid else 8))
    ax = fig.add_subplot(111)
    style = dict(cmap="terrain", vmin=0, vmax=max(args.n_clusters - 1, 1))
    if args.grid:
        ax.imshow(labels, extent=(-180, 180, -90, 90), interpolation="nearest", **style)
    else:
        ax.scatter(locs[:, 0], locs[:, 1], c=labels, s=1, edgecolor="none", **style)
    ax.set_xlabel("longitude")
    ax.set_ylabel("latitude")
    fig.savefig(out + ".png", bbox_inches="tight", dpi=150)
    plt.close(fig)
    print(f"cluster_map: {len(locs)} locations ({info['n_clustered']} clustered), {args.n_clusters} clusters, "
          f"{info['rounds']} linkage rounds -> {out}.npz, {out}.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
