"""The resampler's definition (qwen_tts/resample.py) in plain torch, for the CPU and the GPU tests.

    y[m] = sum_k x[k] * h[m*down - k*up + half]   over the k whose tap index lies in [0, 2*half],  m < ceil(n*up/down)

with x zero outside [0, n).  `resample(x, plan)` evaluates it in `dtype`: float64 on the fp32 taps widened is the
reference, float32 the "plain torch fp32" whose own error scales the GPU tolerance (small_kernel_refs.fp32_tolerance).
torch and numpy only; the plan comes from the caller.
"""
import torch

F32, F64 = torch.float32, torch.float64
RATES = [8000, 12000, 16000, 22050, 32000, 44100, 48000]
# (up, down, filter length, taps per output) at RATES, from 24 kHz: q = max(up, down), half = 10 q
EXPECT = {8000: (1, 3, 61, 61), 12000: (1, 2, 41, 41), 16000: (2, 3, 61, 31), 22050: (147, 160, 3201, 22),
          32000: (4, 3, 81, 21), 44100: (147, 80, 2941, 21), 48000: (2, 1, 41, 21)}
FIRST_PACKET = {8000: 445, 12000: 673, 16000: 900, 22050: 1245, 32000: 1807, 44100: 2490, 48000: 2710}  # after 1365


def _terms(x, plan, dtype, h=None):
    """[M, J] products x[k] * h[tap] of every output (zero where the tap or the sample does not exist)."""
    up, down, half = plan.up, plan.down, plan.half
    h = torch.tensor(plan.h if h is None else h).to(dtype)
    x = torch.as_tensor(x).to(dtype)
    n, L = x.shape[0], 2 * half + 1
    M, J = -(-n * up // down), -(-L // up)
    c = torch.arange(M, dtype=torch.int64)[:, None] * down + half
    k = c // up - torch.arange(J - 1, -1, -1, dtype=torch.int64)[None, :]  # ascending k
    t = c - k * up
    ok = (t < L) & (k >= 0) & (k < n)
    xk = x[k.clamp(0, max(n - 1, 0))] if n else torch.zeros(M, J, dtype=dtype)
    return torch.where(ok, xk * h[t.clamp(0, L - 1)], torch.zeros((), dtype=dtype))


def resample(x, plan, dtype=F64, h=None):
    return _terms(x, plan, dtype, h).sum(-1)


def resample_scale(x, plan):
    """sum_k |x[k] * h[..]| per output: the magnitude the error of a sum of products is measured against"""
    return _terms(x, plan, F64).abs().sum(-1)


def l1_gain(plan):
    """max over phases of sum |h_phase|: how far the filter can amplify a bounded difference of its input"""
    return float(torch.tensor(plan.table).to(F64).abs().sum(-1).max())


def last_needed(plan, M):
    """For each output m < M the largest k with a tap index in [0, 2*half], found by trying every k around m's span"""
    up, down, half = plan.up, plan.down, plan.half
    out = []
    for m in range(M):
        lo, hi = (m * down - half) // up - 2, (m * down + half) // up + 3
        out.append(max(k for k in range(lo, hi) if 0 <= m * down - k * up + half <= 2 * half))
    return out


def brute_ready(plan, n_total, last):
    """Count of outputs m of the signal's ceil(n_total*up/down) whose needed inputs all lie below n_total
    (last = last_needed(plan, M) with M at least that ceiling)."""
    return sum(last[m] < n_total for m in range(-(-n_total * plan.up // plan.down)))


def s16(y):
    return torch.round(y.clamp(-1.0, 1.0) * 32767.0).to(torch.int16)  # torch.round: half to even
