"""Drop-in for the reference's ``src/python/gmmreg_gpu/gmm_impl.py`` (flavour "G": diag only,
KMeans initialisation, no eps inside log(weights), clipped covariance)."""
import numpy as np

from .. import _flat
from .._flat import asarray, timer, DevicePoints  # noqa: F401

eps = 1e-8
VARIANT = "G"


def init_gmm_params(X, k, sample_weight=None):
    """KMeans(k, random_state=1, max_iter=50, n_init=1) centres + uniform weights
    (reference gmm_impl.py:18-24).  The reference calls scikit-learn on the host; here the same
    algorithm (same random stream, same seeds, same stop rule) runs on the device
    (``hgmm_amd.kmeans``, ``csrc/kmeans_kernels.hip``).  ``sample_weight`` (default None: the reference's unweighted
    clustering): ``.fit(X, sample_weight=...)`` as in :meth:`hgmm_amd.kmeans.KMeans.fit`."""
    from ..kmeans import kmeans_centres
    return kmeans_centres(X, k, random_state=1, max_iter=50, sample_weight=sample_weight), np.ones((k)) / k


def init_gmm_params_batch(Xs, k):
    """:func:`init_gmm_params` of every cloud of ``Xs`` through one launch set (``hgmm_amd.kmeans.KMeans.fit_batch``) -> a
    list of its ``(centres, weights)``, member b's bit for bit the serial call's.  Unweighted: the batched initialiser takes no
    ``sample_weight``."""
    from ..kmeans import kmeans_centres_batch
    return [(c, np.ones((k)) / k) for c in kmeans_centres_batch(Xs, k, random_state=1, max_iter=50)]


def estimate_log_prob(X, inv_cov, means):
    """Reference gmmreg_gpu/gmm_impl.py:36-43."""
    return _flat.estimate_log_prob(X, inv_cov, means, 'diag')


def e_step(X, inv_cov, means, weights, sample_weight=None):
    return _flat.e_step(X, inv_cov, means, weights, 'diag', VARIANT, sample_weight)


def m_step(X, resp, centre_hint=None, sample_weight=None):
    return _flat.m_step(X, resp, 'diag', VARIANT, centre_hint, sample_weight)


def train_gmm(X, max_iter, tol, means, covariances, weights=None, sample_weight=None):
    """``sample_weight`` [N] >= 0: per-point weights of the fit (a ``DevicePoints`` may bring its own).  The KMeans seeding of
    :func:`init_gmm_params` does not see them (unless it is handed them: ``init_gmm_params(X, k, sample_weight=)``)."""
    if weights is None:
        weights = np.ones(len(means), dtype=np.float32) / len(means)
    return _flat.train_gmm(X, max_iter, tol, means, covariances, weights, 'diag', VARIANT, sample_weight)


def train_gmm_batch(Xs, max_iter, tol, means, covariances, weights=None, sample_weight=None):
    """B x :func:`train_gmm` in one launch set -> a list of its tuples, member b's bit for bit the serial call's
    (``weights=None``: uniform, as there).  ``sample_weight``: None -- no per-point weights (a member that brings some is
    refused); ``"own"`` -- each member's own; a sequence -- one array or None (its own) per member; ``VoxelCloud`` s of one
    voxel result are fitted count-weighted without a host trip.  J > 1024 runs as a loop of :func:`train_gmm`."""
    if weights is None:
        weights = [np.ones(len(m), dtype=np.float32) / len(m) for m in means]
    if sample_weight is None:
        return _flat.train_gmm_batch(Xs, max_iter, tol, means, covariances, weights, 'diag', VARIANT)
    return _flat.train_gmm_batch(Xs, max_iter, tol, means, covariances, weights, 'diag', VARIANT, sample_weight=sample_weight)


def predict(X, inv_cov, means, weights):
    return _flat.predict(X, inv_cov, means, weights, 'diag', VARIANT)
