"""Builds libpyprob_amd.so (hand-written HIP for gfx950) in-tree with hipcc. No CPU fallback exists: if the
library cannot be built or loaded the package raises."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libpyprob_amd.so')
SOURCES = ['gemm_f32.hip', 'kernels.hip', 'engine.hip', 'panel.hip', 'panel16.hip', 'lstm_input.hip', 'wgrad_t1.hip', 'is_kernels.hip', 'is_step_fused.hip', 'is_step_small.hip', 'obs_embed.hip', 'pack.hip', 'train_loop.hip', 'lstm_tail.hip', 'dp.hip', 'optim.hip', 'dist_kernels.hip', 'cnn2d.hip', 'obs_draw.hip', 'obs_logweight.hip', 'is_batch.hip', 'is_resample.hip', 'is_moments.hip', 'is_hist.hip', 'is_sort.hip', 'is_gmm.hip', 'is_hpd.hip', 'is_psis.hip', 'is_reobserve.hip', 'is_gmm_joint.hip', 'is_kde.hip', 'is_twosample.hip', 'is_pairs.hip', 'is_proposal.hip', 'is_kde_joint.hip', 'is_sinkhorn.hip', 'is_sinkhorn_map.hip']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-Wno-inline-asm']
# Per-source additions. is_gmm_joint.hip: no packed fp32 arithmetic (its float work is loads and conversions to fp64 only).
# is_kde.hip: the same - the P chains of a lane stay scalar fp32 operations, whose roundings the error bound counts one by one.
# is_twosample.hip: the same as is_gmm_joint.hip - its arithmetic is fp64, its floats are compared and converted only.
# is_pairs.hip: the same as is_kde.hip - the distance chain of a pair stays scalar fp32 operations, counted one by one in its bound.
# is_proposal.hip: the same as is_gmm_joint.hip - fp64 arithmetic; its floats are the Box-Muller deviates and conversions.
_NO_PACKED_FP32 = ['-Xclang', '-target-feature', '-Xclang', '-packed-fp32-ops']
EXTRA_FLAGS = {'is_gmm_joint.hip': _NO_PACKED_FP32, 'is_kde.hip': _NO_PACKED_FP32, 'is_twosample.hip': _NO_PACKED_FP32,
               'is_pairs.hip': _NO_PACKED_FP32, 'is_proposal.hip': _NO_PACKED_FP32}


def _hipcc():
    for c in ('/opt/rocm/bin/hipcc', 'hipcc'):
        if os.path.isabs(c) and os.path.exists(c):
            return c
    return 'hipcc'


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


# Kernels whose launches count on TWO workgroups per CU (64-72 KB of LDS each): above 128 VGPRs an 8-wave workgroup gets a CU
# to itself and the launch serialises - the reduction jobs that share `gemm_f32_async_grouped_aux_kernel` with the MFMA tiles
# once pushed it to 169 registers and the config-2 step from 0.114 to 0.175 ms. The compile prints the resource remarks
# (-Rpass-analysis) and the build fails if one of these kernels grows past the limit.
VGPR_LIMITS = {'gemm_f32_async_grouped_aux_kernel': 128, 'gemm_f32_async_grouped_kernel': 128, 'gemm_f32_async_kernel': 128,
               'gemm_f32_async_lstm_kernel': 256}   # (a 4-wave workgroup: two per CU up to 256 VGPRs)


# Kernels that must not touch scratch memory: the joint mixture's tile kernel keeps up to 45 fp64 accumulators, eight particles of
# J floats and their weights in registers (412 VGPRs + AGPRs at J = 8); a private array that lost its static indices would land there.
# The density kernels keep P points (hi, lo, fp32 and fp64 sums) or a 32 x 32 accumulator block per lane, all statically indexed.
# The two-sample merge keeps its heads in LDS and its sums in registers: nothing of it is indexed privately.
# The pair kernels keep a row's fragments or coordinates, a staged column and a 32 x 32 block of exponents, all statically indexed.
# The proposal's particle kernel keeps eight particles of J floats, their Philox words and deviates in registers; its component is LDS's.
# The joint density's main kernel keeps a query's fragments, a staged particle, two 32 x 32 accumulator blocks and five fp64 sums per lane.
# The Sinkhorn half-step keeps a query's fragments, a staged particle, one 32 x 32 accumulator block and one fp64 sum per lane.
# The transport map's main kernel keeps the same with a second accumulator block and five fp64 sums per lane.
NO_SCRATCH = ('joint_tile_kernel', 'kde_tile_kernel', 'kde2d_tile_kernel', 'twosample_tile_kernel', 'pairs_gauss_kernel',
              'pairs_dist_kernel', 'pairs_operand_kernel', 'proposal_particle_kernel', 'proposal_prepare_kernel', 'kdej_main_kernel',
              'kdej_combine_kernel', 'kdej_shift_kernel', 'sink_main_kernel', 'sink_update_kernel', 'map_main_kernel',
              'map_combine_kernel')


def _check_registers(remarks):
    name = None
    for line in remarks.splitlines():
        if 'Function Name:' in line:
            name = line.split('Function Name:')[1].split()[0]
        elif 'VGPRs:' in line and 'AGPRs' not in line and name:
            n = int(line.split('VGPRs:')[1].split()[0])
            for key, limit in VGPR_LIMITS.items():
                if key in name and n > limit:
                    raise RuntimeError('%s uses %d VGPRs (limit %d: two workgroups per CU)' % (name, n, limit))
        elif 'ScratchSize' in line and name and any(key in name for key in NO_SCRATCH):
            if int(line.split(':')[-1].split()[0]) != 0:
                raise RuntimeError('%s uses scratch memory: %s' % (name, line.strip()))


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link the C-ABI shared library. Returns the library path."""
    hipcc = _hipcc()
    import glob
    headers = sorted(glob.glob(os.path.join(CSRC, '*.hpp'))) + [os.path.join(os.path.dirname(HERE), 'include', 'pyprob_amd.h')]
    if not force and not _stale(LIB, [os.path.join(CSRC, s) for s in SOURCES] + headers):
        return LIB      # the prebuilt in-tree library travels to the GPU box; nothing to do
    objdir = os.path.join(HERE, 'build')
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        if force or _stale(o, [s] + headers):
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ['-Rpass-analysis=kernel-resource-usage', '-c', s, '-o', o])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed: %s\n%s' % (' '.join(cmd), r.stderr))
        _check_registers(r.stderr)
        return r

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(objdir, s.replace('.hip', '.o')) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
