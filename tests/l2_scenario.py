"""The multi-start scenario the L2 GMMReg tests share (tests/test_gmmreg_multistart_cpu.py on the host path,
tests/test_gmmreg_resident_gpu.py through a context): the reference's own coarse mixtures of
tests/golden/gmmreg_l2.npz (J = 30, weights x 1e3, kernel width reg_sigma0) with the target centres turned by 60 degrees
about z through their centroid, and the 27 start poses rotation_starts((-60, 0, 60)) about the source centres' centroid.
The truth is the reference's answer on the unturned mixtures (reg_rot, reg_t) composed with the turn."""
import numpy as np

from conftest import load_golden

OPT_MAXITER, OPT_TOL = 10, 1.0e-5


def angle_deg(rot_a, rot_b):
    c = (np.trace(rot_a.T @ rot_b) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def scenario():
    """-> dict: mu_s, phi_s, mu_t, phi_t (the turned target), sigma, starts (27 RigidTransformation), truth_rot."""
    from hgmm_amd.hgmm.hgmm_gpu import rotation_starts
    g = load_golden("gmmreg_l2.npz")
    mu_s, phi_s = g["reg_mu_source"].astype(np.float64), g["reg_phi_source"] * 1e3
    mu_t, phi_t = g["reg_mu_target"].astype(np.float64), g["reg_phi_target"] * 1e3
    a = np.deg2rad(60.0)
    turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = mu_t.mean(axis=0)
    return {"mu_s": mu_s, "phi_s": phi_s, "mu_t": (mu_t - c) @ turn.T + c, "phi_t": phi_t, "sigma": float(g["reg_sigma0"]),
            "starts": rotation_starts((-60, 0, 60), centre=mu_s.mean(axis=0)), "truth_rot": turn @ g["reg_rot"]}


def registration(cost_fn, sc):
    from hgmm_amd.gmmreg_gpu import gmmreg
    return gmmreg.L2DistRegistration(None, None, cost_fn, sigma=sc["sigma"], use_estimated_sigma=False)
