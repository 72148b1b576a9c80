"""Plain references for the learner step's tail (csrc/hrl_optim.hip): the deferred weight-gradient folds with the
norm's block sums, clip_grad_norm_'s rule and Adam.  Everything here is torch on the CPU in fp64 (and, for
adam_emulated, explicit fp32 / fp64 casts); nothing is taken from the kernels' index arithmetic.  The helper's own
tests (tests/test_step_tail_reference.py) pin it against torch and against Python loops.

A fold is the tuple the launch takes, with the partial rows as a CPU tensor:
    (part, stride, col0, nparts, dst, count, mode)
part holds at least (nparts - 1) * stride + col0 + span floats (span = count, 9216 for mode 1); row r's window is
part[r * stride + col0 : r * stride + col0 + span].
"""

import torch

BLOCK = 64                      # elements per norm block (hrl_grad_fold_norm_blocks)
CONV = (9, 32, 32)              # a mode-1 partial row: [tap][ci][co]; its destination is a (co, ci, tap) conv weight


def _window(fold):
    """The fold's partial windows as an (nparts, span) fp64 tensor, in source-column order."""
    part, stride, col0, nparts, dst, count, mode = fold
    span = 9216 if mode == 1 else count
    flat = part.reshape(-1)
    rows = [flat[r * stride + col0:r * stride + col0 + span] for r in range(nparts)]
    return torch.stack(rows).double()


def _to_dst(cols, mode):
    """Values in source-column order -> destination order (last dimension)."""
    if mode == 0:
        return cols
    lead = cols.shape[:-1]
    return cols.view(*lead, *CONV).permute(*range(len(lead)), len(lead) + 2, len(lead) + 1, len(lead)) \
               .reshape(*lead, -1)


def fold_terms64(fold):
    """(sum, sum of |terms|) over the partial rows, fp64, in destination order (count elements each)."""
    w = _window(fold)
    return _to_dst(w.sum(0), fold[6]), _to_dst(w.abs().sum(0), fold[6])


def lane_elements(n, folds):
    """For each position i of the flat buffer, the element whose final value the launch squares at position i.
    A position outside every fold, or inside a mode-0 fold, holds itself.  Position dst + j of a mode-1 fold reads
    source column j, whose sum belongs to the element the (tap, ci, co) -> (co, ci, tap) transposition sends it to:
    the block sums partition the buffer (every element counted once), but a mode-1 fold's elements are grouped by
    source column, not by destination."""
    holds = torch.arange(n)
    for part, stride, col0, nparts, dst, count, mode in folds:
        if mode == 1:
            # element index written by source column (tap, ci, co): the (co, ci, tap) numbering seen from (tap, ci, co)
            holds[dst:dst + count] = dst + torch.arange(count).view(32, 32, 9).permute(2, 1, 0).reshape(-1)
    return holds


def block_sums64(values, n, folds):
    """fp64 sum of squares of `values` (fp32 values, any float dtype) per 64-position block, each position
    contributing the element lane_elements names."""
    v = values.double()[lane_elements(n, folds)]
    nb = (n + BLOCK - 1) // BLOCK
    pad = torch.zeros(nb * BLOCK, dtype=torch.float64)
    pad[:n] = v * v
    return pad.view(nb, BLOCK).sum(1)


def fold64(flat, folds):
    """(new flat buffer in fp64, block sums): flat[dst + j] += the fp64 sum over the fold's partial rows (mode 0:
    column j; mode 1: the [tap][ci][co] row transposed to (co, ci, tap)); the block sums are of the fp32-rounded
    result."""
    new = flat.double().clone()
    for fold in folds:
        s, _ = fold_terms64(fold)
        dst, count = fold[4], fold[5]
        new[dst:dst + count] += s
    return new, block_sums64(new.float(), flat.numel(), folds)


def clip64(g, max_norm, dtype=torch.float32):
    """clip_grad_norm_'s rule: (g * coef in fp64, total, coef).  The norm is formed in fp64 and rounded to `dtype`;
    coef = max_norm / (total + 1e-6) in `dtype`, clamped to at most 1 with NaN propagating (torch.clamp).  dtype is
    the gradients' own type, as in torch: fp32 for the kernels, fp64 when the rule itself is compared with torch on
    fp64 parameters."""
    total = g.double().pow(2).sum().sqrt().to(dtype)
    coef = torch.tensor(max_norm, dtype=dtype) / (total + torch.tensor(1e-6, dtype=dtype))
    coef = torch.clamp(coef, max=1.0)
    return g.double() * coef.double(), total, coef


def adam64(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0):
    """The textbook Adam step in fp64 (L2 weight decay, bias corrections, eps outside the square root: torch's
    ADAM_MODE::ORIGINAL).  `step` is the count after this step.  Returns (p, m, v)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if wd != 0:
        g = g + wd * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - (lr / bc1) * m / denom, m, v


def adam_emulated(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0):
    """The same step with the promotions include/hrl_nn.h promises (ATen fused_adam_utils.cuh adam_math): p, g, m, v
    fp32 tensors, lr and step fp32 values; moments and the weight-decayed gradient formed in double and rounded to
    float, bias corrections in double handed over as floats, the square root, the quotients and the update in
    float.  Returns fp32 (p, m, v)."""
    f32 = lambda x: torch.as_tensor(x, dtype=torch.float64).float()
    p, g, m, v = p.float(), g.float(), m.float(), v.float()
    stepd = float(f32(step))
    bc1 = f32(1.0 - beta1 ** stepd)
    bc2s = f32((1.0 - beta2 ** stepd) ** 0.5)
    step_size = f32(float(f32(lr)) / float(bc1))
    if wd != 0:
        g = (g.double() + p.double() * wd).float()
    m = (beta1 * m.double() + (1 - beta1) * g.double()).float()
    v = (beta2 * v.double() + (1 - beta2) * g.double() * g.double()).float()
    denom = ((v.sqrt() / bc2s).double() + eps).float()
    return p - step_size * m / denom, m, v
