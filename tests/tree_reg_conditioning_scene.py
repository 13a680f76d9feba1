"""The scene of the conditioning ladder (test_tree_reg_conditioning_cpu.py, test_tree_reg_conditioning_gpu.py): a tree of
one level whose eight centroids lie within ``delta`` of a line, so that the rotation about that line is determined only to
the order delta^2 and the registration's 6 x 6 normal equations lose their smallest eigenvalue with it.

  nodes    L = 1, eight isotropic nodes, sigma = 0.02, pi = 1/8, means (0.1 i, delta cos 2.4 i, delta sin 2.4 i)
  target   32 points per node, each the node's mean plus N(0, 0.01^2) along x only (the points of a node share its y and
           z exactly: the centroid of what a node receives is off the line by what the node's mean is), then moved by one
           degree about z and (0.002, -0.001, 0.001)

lambda_min / lambda_max of the oracle's A^T A at the start pose falls as delta^2 (8.4e-5 at delta = 1e-2).  The smallest
Cholesky pivot over the largest diagonal entry falls only as delta: unpivoted Cholesky is not rank-revealing."""
import numpy as np

from oracle import hgmm_tree

L = 1
LC = 0.01
SIGMA = 0.02
PER_NODE = 32
SEED = 5
COND_RULE = 1e-11                      # reg_host_step: lambda_min <= 1e-11 lambda_max hands the iteration over
LADDER = (1e-2, 1e-4, 1e-6, 1e-7, 3e-8, 1e-9)
I3, Z3 = np.identity(3), np.zeros(3)


def rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def scene(delta):
    """-> (pi [8], mu [8,3], cov [8,3,3], target [256,3]) for one rung of the ladder."""
    i = np.arange(8, dtype=np.float64)
    mu = np.stack([0.1 * i, delta * np.cos(2.4 * i), delta * np.sin(2.4 * i)], axis=1)
    pi = np.full(8, 1.0 / 8)
    cov = np.tile(SIGMA ** 2 * np.identity(3), (8, 1, 1))
    rs = np.random.RandomState(SEED)
    pts = np.repeat(mu, PER_NODE, axis=0)
    pts[:, 0] += 0.01 * rs.randn(len(pts))
    target = pts @ rot_z(1.0).T + np.array([0.002, -0.001, 0.001])
    return pi, mu, cov, target


def oracle_system(pi, mu, cov, target, rot=I3, t=Z3):
    """The oracle's moments and normal equations at pose (rot, t): -> (m0, A^T A, A^T b)."""
    m0, m1, _ = hgmm_tree.reg_e_step(target @ rot.T + t, pi, mu, cov, L, LC)
    ata, atb = hgmm_tree.reg_normal_equations(m0, m1, mu, cov)[:2]
    return m0, ata, atb


def eig_ratio(ata):
    lam = np.linalg.eigvalsh(ata)
    return lam[0] / lam[-1]


def pivot_ratio(ata):
    """Smallest pivot of the unpivoted Cholesky factorisation (the squares of the factor's diagonal) over the largest
    diagonal entry: what reg_device_step tested before it shared the host's rule.  0 where the factorisation breaks down."""
    try:
        piv = np.diag(np.linalg.cholesky(ata)) ** 2
    except np.linalg.LinAlgError:
        return 0.0
    return piv.min() / np.diag(ata).max()


def hands_over(delta):
    """The oracle's verdict for a rung: True where lambda_min <= 1e-11 lambda_max at the start pose."""
    return eig_ratio(oracle_system(*scene(delta))[1]) <= COND_RULE
