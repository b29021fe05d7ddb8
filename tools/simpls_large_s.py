"""Time pls_regression past the on-chip bound on S (the global route of the SIMPLS component-step kernels).

    python tools/simpls_large_s.py [--quick]

For S = 24 000 (B = 2000, T = 10, k = 10) and S = 48 000 (B = 400, T = 4, k = 3): one warm-up call, then one timed
call of the public pls_regression with n_perm + n_boot resamples on a fixed-budget engine.  Prints one JSON line
per shape: resamples/s of the whole call, the share of the call spent in the products with K (k_nt_gemm, the
formation of K included) and in the solver kernels of the component steps (k_sd_*), and the products' fp64 rate
against the measured MFMA peak.  DESIGN.md section 5 records the results."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(S, B, T, k, n, seed=0):
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, seed=seed + 1, verbose=False, _engine=eng)
    pls.pls_regression(X, Y, n_perm=8, n_boot=8, **kw)            # warm-up: code objects, scratch
    torch.cuda.synchronize()
    eng.set_timing(True)
    t0 = time.perf_counter()
    pls.pls_regression(X, Y, n_perm=n, n_boot=n, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kt = eng.kernel_timing()
    flops = eng.last_timing().get('nt_flops', 0.0)
    eng.set_timing(False)
    nt_ms = kt.get('k_nt_gemm', (0.0, 0))[0]
    sd_ms = kt.get('k_simpls_dual', (0.0, 0))[0]
    peak = eng.mfma_f64_peak()
    return dict(S=S, B=B, T=T, k=k, n_perm=n, n_boot=n, seconds=round(wall, 3),
                resamples_per_s=round(2 * n / wall, 1), ms_per_resample=round(1e3 * wall / (2 * n), 3),
                nt_share=round(nt_ms / (1e3 * wall), 3), solver_share=round(sd_ms / (1e3 * wall), 3),
                nt_ms=round(nt_ms, 1), solver_ms=round(sd_ms, 1),
                nt_tflops=round(flops / (nt_ms * 1e9), 2) if nt_ms > 0 else None,
                mfma_f64_peak_tflops=round(peak, 1), kernel_ms={key: round(v[0], 2) for key, v in kt.items()})


def main():
    quick = '--quick' in sys.argv
    for S, B, T, k, n in ((24000, 2000, 10, 10, 200 if quick else 1000), (48000, 400, 4, 3, 100 if quick else 500)):
        print(json.dumps(run(S, B, T, k, n)), flush=True)


if __name__ == '__main__':
    main()
