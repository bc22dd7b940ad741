#!/usr/bin/env python3
"""k-NN graph of a data set on the GPU: every stored row queried against the index it is stored in, the row itself
left out (IVF.knn_graph).

    python examples/knn_graph.py --input random-200000-64 --k 10 --n-probes 10
"""
import argparse
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyknn_amd import IVF, FastPQ, utils                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--input", default="random-200000-64", help=".npy file or random-n-d")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--n-probes", type=int, default=10)
ap.add_argument("--clusters", type=int, default=400)
args = ap.parse_args()

m = re.match(r"random-(\d+)-(\d+)", args.input)
np.random.seed(10)
X = np.random.randn(*map(int, m.groups())).astype(np.float32) if m else np.load(args.input).astype(np.float32)
with utils.timer(True, "Fitting and building"):
    ivf = IVF("euclidean", args.clusters, FastPQ(2)).fit(X[:10**5]).build(X, n_probes=1)
with utils.timer(True, "k-NN graph"):
    ids, dists = ivf.knn_graph(args.k, n_probes=args.n_probes, return_distances=True)
assert not (ids == np.arange(len(X))[:, None]).any()       # no row is its own neighbour
print("rows:", len(X), "edges:", int((ids != -1).sum()), "mean distance to the nearest:", float(dists[:, 0].mean()))
