"""pyprob_amd: MI355X-native inference-compilation engine behind pyprob's InferenceNetworkLSTM / importance-sampling
API. Hand-written HIP (gfx950) behind a C ABI (include/pyprob_amd.h); PyTorch-ROCm is used for HBM allocation,
streams and torch.distributed only."""
__version__ = '0.1.0'

# the posterior statistics over a list of posteriors and their result types (empirical_batch.py, empirical.py)
_FROM_DISTRIBUTIONS = frozenset((
    'resample_batch', 'joint_batch', 'histogram_batch', 'quantile_batch', 'hpd_batch', 'cdf_batch', 'pareto_k_batch', 'psis_batch',
    'density_estimate_batch', 'reobserve_batch', 'Histogram', 'Histogram2D', 'MixtureFit', 'PsisFit'))


def __getattr__(name):
    """Lazy pyprob-style top level: pyprob_amd.sample / observe / Model / InferenceEngine / PriorInflation ... (importing the package
    must not require torch or a GPU)."""
    if name in ('sample', 'observe', 'factor', 'TraceMode', 'InferenceEngine', 'PriorInflation', 'InferenceNetwork', 'LearningRateScheduler',
                'Optimizer'):
        from . import state
        value = getattr(state, name)
        globals()[name] = value          # (resolved once: `pyprob.sample(...)` in a program runs per statement and per path)
        return value
    if name == 'ObserveEmbedding':
        from .spec import ObserveEmbedding
        globals()[name] = ObserveEmbedding
        return ObserveEmbedding
    if name in _FROM_DISTRIBUTIONS:
        from . import distributions
        value = getattr(distributions, name)
        globals()[name] = value
        return value
    if name == 'Model':
        from .model import Model
        globals()[name] = Model
        return Model
    raise AttributeError(name)
