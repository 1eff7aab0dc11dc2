"""Float64 restatement of the exposure affine (``mvs_gaussian_splatting_amd/exposure.py``, ``csrc/exposure.hip``) in
torch, from the float32 inputs cast to double.  Image ``x [3,H,W]``, exposure ``A [3,4]``, ``g = dL/dy``; ``k`` is the
input channel, ``c`` the output channel:

    y[c,p]  = x[0,p]*A[0,c] + x[1,p]*A[1,c] + x[2,p]*A[2,c] + A[c,3]
    dx[k,p] = A[k,0]*g[0,p] + A[k,1]*g[1,p] + A[k,2]*g[2,p]
    dA[k,c] = sum_p x[k,p]*g[c,p]        dA[c,3] = sum_p g[c,p]

Each function also returns the sum of the magnitudes of the terms of every result: what the rounding bars of
tests/test_gpu_exposure.py scale with.  Shared by tests/test_exposure_host.py and tests/test_gpu_exposure.py.
"""
import torch

U = 2.0 ** -24            # unit roundoff of float32
A_TRUE = [[1.20, 0.05, 0.00, -0.05], [0.00, 0.90, 0.03, 0.02], [-0.04, 0.00, 1.10, 0.04]]


def _f64(t):
    return t.detach().cpu().to(torch.float64)


def forward64(x, A):
    """-> (y, sum_k |x_k A_kc| + |A_c3|), both float64 ``[3,H,W]`` on the CPU."""
    x, A = _f64(x), _f64(A)
    y = torch.stack([x[0] * A[0, c] + x[1] * A[1, c] + x[2] * A[2, c] + A[c, 3] for c in range(3)])
    mag = torch.stack([(x[0] * A[0, c]).abs() + (x[1] * A[1, c]).abs() + (x[2] * A[2, c]).abs() + A[c, 3].abs()
                       for c in range(3)])
    return y, mag


def backward64(x, A, g):
    """-> (dx, sum_c |A_kc g_c|, dA, sum_p |term|): float64; dx and its scale ``[3,H,W]``, dA and its scale ``[3,4]``."""
    x, A, g = _f64(x), _f64(A), _f64(g)
    dx = torch.stack([A[k, 0] * g[0] + A[k, 1] * g[1] + A[k, 2] * g[2] for k in range(3)])
    dx_mag = torch.stack([(A[k, 0] * g[0]).abs() + (A[k, 1] * g[1]).abs() + (A[k, 2] * g[2]).abs() for k in range(3)])
    dA = torch.zeros(3, 4, dtype=torch.float64)
    dA_mag = torch.zeros(3, 4, dtype=torch.float64)
    for c in range(3):
        for k in range(3):
            dA[k, c] = (x[k] * g[c]).sum()
            dA_mag[k, c] = (x[k] * g[c]).abs().sum()
        dA[c, 3] = g[c].sum()
        dA_mag[c, 3] = g[c].abs().sum()
    return dx, dx_mag, dA, dA_mag
