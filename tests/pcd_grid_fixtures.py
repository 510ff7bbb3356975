"""Seeded clouds shared by tests/test_pcd_grid_cpu.py and tests/test_pcd_grid_gpu.py: the shapes a uniform grid handles worst."""
import numpy as np


def lattice(seed=0):
    """The 17 x 17 x 3 integer lattice in shuffled order, and queries at its cell centres and at its points."""
    g = np.stack(np.meshgrid(np.arange(17.0), np.arange(17.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)
    t = g[np.random.default_rng(seed).permutation(len(g))]
    c = np.stack(np.meshgrid(np.arange(16.0) + 0.5, np.arange(16.0) + 0.5, np.arange(2.0) + 0.5, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([c, g], 0), t


def planar(n=1500, seed=1):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-2.0, 2.0, (n, 2)), np.full((n, 1), 0.75)], 1)


def cluster(n=4000, seed=2):
    """90 % of the points inside a 1e-3 box, the rest spread over a 10 m box."""
    rng = np.random.default_rng(seed)
    k = n * 9 // 10
    p = np.concatenate([rng.uniform(0.0, 1e-3, (k, 3)) + 4.0, rng.uniform(0.0, 10.0, (n - k, 3))], 0)
    return p[rng.permutation(n)]
