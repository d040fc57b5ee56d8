"""Builds libpyprob_amd.so (hand-written HIP for gfx950) in-tree with hipcc. No CPU fallback exists: if the
library cannot be built or loaded the package raises."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libpyprob_amd.so')
SOURCES = ['gemm_f32.hip', 'kernels.hip', 'engine.hip', 'panel.hip', 'panel16.hip', 'lstm_input.hip', 'wgrad_t1.hip', 'is_kernels.hip', 'is_step_fused.hip', 'is_step_small.hip', 'obs_embed.hip', 'pack.hip', 'train_loop.hip', 'lstm_tail.hip', 'dp.hip', 'optim.hip', 'dist_kernels.hip', 'cnn2d.hip', 'obs_draw.hip', 'obs_logweight.hip', 'is_batch.hip', 'is_resample.hip', 'is_moments.hip', 'is_hist.hip', 'is_sort.hip', 'is_gmm.hip', 'is_hpd.hip', 'is_psis.hip', 'is_reobserve.hip']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-Wno-inline-asm']


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
            jobs.append([hipcc] + FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', s, '-o', o])

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
