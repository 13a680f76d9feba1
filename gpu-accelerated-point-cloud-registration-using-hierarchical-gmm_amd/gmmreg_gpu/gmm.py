"""Drop-in for the reference's ``src/python/gmmreg_gpu/gmm.py`` (flavour "G"): ``compute``
returns ``(means, weights)`` only (reference gmm.py:57,70); covariances start at 0.1
(gmm.py:80); host NumPy results (gmm.py:95)."""
import numpy as np

from ..gmm_waymo.gmm import Feature, GMM_Sklearn, _cpu_name_notice, _split_weighted, _Weighted  # noqa: F401
from ..gmm_waymo.gmm import OneClassSVM as _SklearnOneClassSVM
from . import gmm_impl
from .gmm_impl import train_gmm, train_gmm_batch, init_gmm_params, init_gmm_params_batch, timer, predict, asarray  # noqa: F401
from .gmm_impl import DevicePoints


class GMM_GPU_Base:
    _label = 'GPU GMM TRAIN'

    def __init__(self, num_components, max_iter=30, tol=1e-4, weighted_init=False):
        """``weighted_init=True`` (an option of the estimator, so that ``fit`` keeps its argument list): the KMeans seeding
        gets the same per-point weights as the EM; a fit without weights is then refused."""
        self.num_components = num_components
        self.max_iter = max_iter
        self.tol = tol
        self.weighted_init = bool(weighted_init)

    def fit(self, X, init=None, sample_weight=None):
        """``sample_weight`` [N] >= 0 (default None; a ``WeightedPoints(points, weights)`` brings its own): point i counts as
        that many points.  The KMeans seeding of ``init_gmm_params`` does not see the weights -- unless the estimator was
        built with ``weighted_init=True``: the seeding then gets the same weights as the EM (refused without weights)."""
        X, sample_weight = _split_weighted(X, sample_weight)
        if self.weighted_init and sample_weight is None:
            raise ValueError("weighted_init=True needs per-point weights (sample_weight=, or a WeightedPoints input)")
        X = np.asarray(X)
        dev_X = asarray(X.astype(np.float32), weights=sample_weight)         # (the weights travel with the resident cloud)
        if init is not None:
            means, weights = init
        elif self.weighted_init:
            means, weights = init_gmm_params(X, self.num_components, sample_weight=sample_weight)
        else:
            means, weights = init_gmm_params(X, self.num_components)
        covs = 0.1 * np.ones((self.num_components, 3), dtype=np.float32)
        with timer(self._label):
            inv, mu, w, cov, lls = train_gmm(dev_X, self.max_iter, self.tol, np.asarray(means, np.float32),
                                             covs, np.asarray(weights, np.float32))
        self.means_, self.covariances_, self.weights_ = mu, cov, w
        self.lls, self.inv_covs = lls, inv
        if len(lls):
            print("\nLog Likelihood Min-Max:\n\n", np.min(lls), np.max(lls))
        return self

    def fit_batch(self, frames, inits=None, sample_weight=None):
        """One fit per frame through ONE launch set each for the initialiser (``init_gmm_params_batch``: the batched KMeans)
        and for the EM (``train_gmm_batch``) -> a list of fitted estimators of this one's settings, each bit for bit in the
        state ``.fit(frame)`` leaves one in (this estimator itself stays as it is).  ``inits``: one ``(means, weights)`` per
        frame instead of the initialiser.

        ``sample_weight``: the convention of ``gmm_waymo``'s ``fit_batch`` -- None: frames that bring per-point weights are
        refused; ``"own"``: each frame's own; a sequence: one array or None (its own) per frame.  The initialiser does not see
        the weights, and an estimator built with ``weighted_init=True`` is refused: the batched initialiser is unweighted."""
        if self.weighted_init:
            raise ValueError("fit_batch: weighted_init=True is not supported -- the batched KMeans initialiser is unweighted; "
                             "fit the frames one by one with fit(frame)")
        frames = list(frames)
        if inits is not None and len(inits) != len(frames):
            raise ValueError("fit_batch: %d frames, but %d initialisations" % (len(frames), len(inits)))
        if sample_weight is not None and not isinstance(sample_weight, str) and len(sample_weight) != len(frames):
            raise ValueError("fit_batch: %d frames, but %d sample_weight entries" % (len(frames), len(sample_weight)))
        clouds, hosts = [], []
        for b, X in enumerate(frames):
            if sample_weight is None and getattr(X, "weights", None) is not None:
                raise ValueError("fit_batch: frame %d brings per-point weights, which the batched fit does not take unless the "
                                 "call says so: pass sample_weight='own', or fit it with fit(frame)" % b)
            P, _ = _split_weighted(X, None)
            host = P.get() if isinstance(P, DevicePoints) else np.asarray(P)
            hosts.append(host)
            if sample_weight is None or isinstance(P, DevicePoints):
                clouds.append(P if isinstance(P, DevicePoints) else host.astype(np.float32))
            else:                                                # (a WeightedPoints keeps its weights on the way down)
                clouds.append(_Weighted(host.astype(np.float32), getattr(X, "weights", None)))
        if not frames:
            return []
        params = list(inits) if inits is not None else init_gmm_params_batch(hosts, self.num_components)
        covs = [0.1 * np.ones((self.num_components, 3), dtype=np.float32) for _ in frames]
        with timer(self._label):
            extra = {} if sample_weight is None else {"sample_weight": sample_weight}
            fits = train_gmm_batch(clouds, self.max_iter, self.tol, [np.asarray(p[0], np.float32) for p in params], covs,
                                   [np.asarray(p[1], np.float32) for p in params], **extra)
        models = []
        for inv, mu, w, cov, lls in fits:
            m = type(self)(self.num_components, self.max_iter, self.tol)
            m.means_, m.covariances_, m.weights_ = mu, cov, w
            m.lls, m.inv_covs = lls, inv
            if len(lls):
                print("\nLog Likelihood Min-Max:\n\n", np.min(lls), np.max(lls))
            models.append(m)
        return models

    def predict(self, X):
        return predict(np.asarray(X).astype(np.float32), self.inv_covs, self.means_, self.weights_)


class GMM_CPU_Base(GMM_GPU_Base):
    """The reference's GMM_CPU_Base.fit is broken (unpacks 3 values from a 2-tuple,
    gmmreg_gpu/gmm.py:117); this one works and, like everything here, runs on the GPU engine."""
    _label = 'CPU GMM TRAIN'

    def __init__(self, *args, **kwargs):
        _cpu_name_notice("GMM_CPU_Base")
        super().__init__(*args, **kwargs)


class GMM_GPU(Feature):
    _base = GMM_GPU_Base

    def __init__(self, n_gmm_components=100, max_iter=30, tol=1e-4, weighted_init=False):
        self._n_gmm_components = n_gmm_components
        self.max_iter = max_iter
        self.tol = tol
        self.weighted_init = bool(weighted_init)

    def init(self):
        if self.weighted_init:
            self._clf = self._base(self._n_gmm_components, max_iter=self.max_iter, tol=self.tol, weighted_init=True)
        else:
            self._clf = self._base(self._n_gmm_components, max_iter=self.max_iter, tol=self.tol)

    def compute(self, data, weights=None):
        """``weights`` [N] >= 0: per-point weights of the fit; a ``WeightedPoints`` brings its own.  The KMeans seeding does
        not see the weights unless the feature was built with ``weighted_init=True`` (then refused without weights)."""
        self._clf.fit(data, sample_weight=weights)
        return self._clf.means_, self._clf.weights_

    def predict(self, data):
        return self._clf.predict(data)


class GMM_CPU(GMM_GPU):
    _base = GMM_CPU_Base


class OneClassSVM(_SklearnOneClassSVM):
    """reference gmmreg_gpu/gmm.py:141-167.  That file imports the third-party ``thundersvm`` at module
    level (gmm.py:12) but builds the estimator from scikit-learn's ``svm.OneClassSVM`` (gmm.py:158), which
    is what this class does; ``RigidSVR`` / ``registration_svr`` (gmmreg.py:123-136, 159-169) use it."""
