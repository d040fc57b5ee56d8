"""Records tests/golden/gmm_sklearn.npz: the reference's own Empirical(values).density_estimate(K, weights_init=, means_init=,
precisions_init=) - pyprob forwards the keyword arguments to scikit-learn's GaussianMixture(covariance_type='diag') - on four
integer-weighted cases, each value REPEATED by its multiplicity (the reference has no sample weights: an unweighted Empirical is
fitted on all its values). Stored per case c: c_values (float32), c_mult (the multiplicities 1 .. 5), c_init (weights | means |
variances the fit started from), c_fit (weights | means | variances it ended with), c_n_iter, c_lower_bound. tests/gmm_ref.py must
reproduce it from (values, log(mult)). Run on the build machine only (needs the reference next to the repository and
scikit-learn):  python tests/golden/make_gmm_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('PYPROB_REFERENCE', '/root/reference')

CASES = {'k1': (1, 1500), 'k2': (2, 3000), 'k3': (3, 4000), 'k5': (5, 4000)}      # name: (K, n)


def make_case(rng, K, n):
    """n float32 values from K well separated modes, multiplicities 1 .. 5, and a start that is not the answer."""
    centres = np.linspace(-2.0, 2.0 * K, K) if K > 1 else np.array([1.5])
    comp = rng.integers(0, K, n)
    values = (centres[comp] + rng.normal(0.0, 0.35, n) * (1.0 + 0.5 * comp / max(K - 1, 1))).astype(np.float32)
    mult = rng.integers(1, 6, n)
    w = rng.uniform(0.5, 1.5, K)
    init = np.concatenate([w / w.sum(), centres + rng.normal(0.0, 0.3, K), rng.uniform(0.2, 0.6, K)])
    return values, mult, init


def main():
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, REFERENCE)
    import sklearn.mixture as skm
    from pyprob.distributions import Empirical
    fitted = []
    fit = skm.GaussianMixture.fit

    def recording_fit(self, X, y=None):      # (density_estimate returns the Mixture only: n_iter_ and lower_bound_ stay on the estimator)
        out = fit(self, X, y)
        fitted.append(self)
        return out
    skm.GaussianMixture.fit = recording_fit
    rng = np.random.default_rng(20240607)
    store = {}
    for name, (K, n) in CASES.items():
        values, mult, init = make_case(rng, K, n)
        repeated = np.repeat(values, mult)
        mix = Empirical(values=[float(v) for v in repeated]).density_estimate(
            K, weights_init=init[:K], means_init=init[K:2 * K].reshape(K, 1), precisions_init=(1.0 / init[2 * K:]).reshape(K, 1))
        m = fitted[-1]
        assert m.converged_ and len(mix.distributions) == K
        store[name + '_values'], store[name + '_mult'], store[name + '_init'] = values, mult.astype(np.int32), init
        store[name + '_fit'] = np.concatenate([m.weights_, m.means_[:, 0], m.covariances_[:, 0]])
        store[name + '_n_iter'], store[name + '_lower_bound'] = np.int32(m.n_iter_), np.float64(m.lower_bound_)
        print(name, 'K', K, 'n', n, 'repeated', len(repeated), 'n_iter', m.n_iter_, 'lower_bound', m.lower_bound_)
    path = os.path.join(HERE, 'gmm_sklearn.npz')
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
