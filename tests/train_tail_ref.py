"""CPU references and comparisons for the kernels that close a training step: the label-smoothed cross entropy and its gradient (csrc/decoder.hip, csrc/loss_bwd.hip),
the token-embedding forward and gradient, and the flat-buffer AdamW step (csrc/train_ops.hip).  Plain torch in fp64, written from the formulas, no GPU.

    loss[b, u]   = (1 - eps) (lse(z) - z[t]) + eps (lse(z) - mean(z)),        t = labels[b, u + shift]   (t < 0: the row is ignored),  z = logits[b, u, :V]
    dlogits[b, u, c] = k (softmax(z)[c] - eps / V - (1 - eps) [c == t]),      k = weight / count,  count = the number of rows that are not ignored
    dwte[ids[m]] += scale dx[m] (ids outside [0, V) add nothing);  dwpe[pos_offset + m % U] += dx[m];   out[m] = scale wte[clamp(ids[m], 0, V - 1)] + pos[pos_offset + m % U]

Tests with sums in them use `int_valued` inputs: every partial sum is then an integer multiple of one power of two below 2**24 of them, hence exact in fp32 in ANY order,
and the device result must EQUAL the fp64 one — a dropped or doubled row cannot hide under a rounding bound."""
import numpy as np
import torch

F64 = torch.float64
BF16 = torch.bfloat16
TINY = 2.0 ** -126          # the smallest normal fp32 / bf16 magnitude: below it the hardware exponential returns zero


# ---------------------------------------------------------------------------------------------------------------- cross entropy
def ce_ref(logits_f32, labels, shift, eps, weight, count=None, ldo=None):
    """logits (B, U, V) fp32 (any strides; only the V columns are read), labels (B, U) int64.  count: the caller's own denominator (the [sum, count] pair the gradient
    kernel is handed need not come from the forward); None: the number of valid rows.  Everything returned is fp64:
        row_loss (B * (U - shift))  NaN on ignored rows        acc [sum of the valid rows' losses, their number]
        grad (B * U, ldo)           the layout of the gradient kernel's output: ignored rows, the last `shift` rows of every utterance and columns V.. are zero
        p (B * U, V) softmax        target (B * U) int64, -100 where the row has no gradient        k, eps, V"""
    B, U, V = logits_f32.shape
    ldo = V if ldo is None else ldo
    z = logits_f32.detach().cpu().to(F64)
    lab = labels.detach().cpu().long()
    tgt = torch.full((B, U), -100, dtype=torch.long)
    tgt[:, :U - shift] = lab[:, shift:]
    tgt = torch.where(tgt < 0, torch.full_like(tgt, -100), tgt).reshape(B * U)
    z = z.reshape(B * U, V)
    lse = torch.logsumexp(z, dim=1)
    p = torch.exp(z - lse[:, None])
    valid = tgt >= 0
    safe = tgt.clamp(min=0)
    loss = (1.0 - eps) * (lse - z.gather(1, safe[:, None])[:, 0]) + eps * (lse - z.mean(dim=1))
    loss = torch.where(valid, loss, torch.full_like(loss, float("nan")))
    n_valid = int(valid.sum())
    acc = torch.tensor([float(loss[valid].sum()), float(n_valid)], dtype=F64)
    row_loss = loss.reshape(B, U)[:, :U - shift].reshape(-1)
    cnt = float(n_valid) if count is None else float(count)
    k = weight / cnt if cnt > 0 else 0.0
    onehot = torch.zeros(B * U, V, dtype=F64)
    onehot[valid, safe[valid]] = 1.0
    g = k * (p - eps / V - (1.0 - eps) * onehot)
    g[~valid] = 0.0
    grad = torch.zeros(B * U, ldo, dtype=F64)
    grad[:, :V] = g
    return dict(row_loss=row_loss, acc=acc, grad=grad, p=p, target=tgt, k=k, eps=float(eps), V=V, ldo=ldo)


def ce_grad_tol(ref):
    """(B * U, V) fp64:  2**-8 |want| + 2**-16 k (p + eps / V + [c == target]) + 2**-126.
    First term: one bf16 ulp of the stored value.  Second: forward error of the fp32 evaluation relative to the SUM of the magnitudes of the terms that cancel in it
    (the hardware exponential at x - max ~ -20 is good to ~2e-6 relative; 2**-16 leaves ~8x).  Third: neither fp32 nor bf16 holds anything between zero and its
    subnormals — a softmax term of e**-160 (a row with logits +80 and -80, eps = 0) has no representation, and exponentials below 2**-126 flush to zero; it is 1e-30
    of any gradient that matters."""
    V = ref["V"]
    want = ref["grad"][:, :V]
    onehot = torch.zeros_like(want)
    valid = ref["target"] >= 0
    onehot[valid, ref["target"][valid]] = 1.0
    return 2.0 ** -8 * want.abs() + 2.0 ** -16 * ref["k"] * (ref["p"] + ref["eps"] / V + onehot) + TINY


def ce_grad_report(got, ref):
    """elementwise, no element exempt.  got (B * U, ldo) bf16 (or any float dtype).  Returns dict(ok, worst = max err / tol over the rows that carry a gradient, n_bad,
    first = (row, column, got, want) of the worst element, zeros_ok = rows without a gradient and columns V.. are exactly zero)"""
    V = ref["V"]
    got = got.detach().cpu().to(F64)
    assert got.shape == ref["grad"].shape, (got.shape, ref["grad"].shape)
    active = ref["target"] >= 0
    if ref["k"] == 0.0:
        active = torch.zeros_like(active)
    must_zero = torch.ones_like(got, dtype=torch.bool)
    must_zero[active, :V] = False
    zeros_ok = bool((got[must_zero] == 0).all())                 # NaN != 0: poison that survives fails here
    want = ref["grad"][:, :V]
    err = (got[:, :V] - want).abs()
    ratio = err / ce_grad_tol(ref)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)[active]
    if ratio.numel() == 0:
        return dict(ok=zeros_ok, worst=0.0, n_bad=0, first=None, zeros_ok=zeros_ok)
    worst = float(ratio.max())
    rows = torch.nonzero(active)[:, 0]
    i = int(ratio.argmax())
    r, c = int(rows[i // V]), i % V
    return dict(ok=zeros_ok and worst <= 1.0, worst=worst, n_bad=int((ratio > 1.0).sum()), zeros_ok=zeros_ok,
                first=(r, c, float(got[r, c]), float(want[r, c])))


def ce_grad_ok(got_bf16, ref):
    return ce_grad_report(got_bf16, ref)["ok"]


def ce_grad_emulated_f32(logits_f32, ref):
    """the gradient kernel's own formula in fp32, NOT rounded to bf16: max, exp(x - max), sum, one reciprocal, k * (e * inv - eps / V - (1 - eps) [c == t])"""
    V = ref["V"]
    x = logits_f32.detach().cpu().float().reshape(-1, V)
    mx = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - mx)
    inv = 1.0 / e.sum(dim=1, keepdim=True)
    k, sm, hot = torch.tensor(ref["k"], dtype=torch.float32), torch.tensor(ref["eps"] / V, dtype=torch.float32), torch.tensor(1.0 - ref["eps"], dtype=torch.float32)
    valid = ref["target"] >= 0
    onehot = torch.zeros_like(x)
    onehot[valid, ref["target"][valid]] = 1.0
    g = k * (e * inv - sm - onehot * hot)
    g[~valid] = 0.0
    out = torch.zeros(x.shape[0], ref["ldo"], dtype=torch.float32)
    out[:, :V] = g
    return out


def old_floor_close_ok(got, want, rel=1.2e-2, floor=5e-3):
    """the comparison tests/test_gpu_train_ops.py::test_ce_and_embed_bwd made of the CE gradient before it was replaced by `ce_grad_ok`:
    |got - want| <= floor * max|want| + rel * |want|.  Kept to show what it lets through."""
    got, want = got.float(), want.float()
    return bool(((got - want).abs() <= floor * want.abs().max() + rel * want.abs()).all())


# ---------------------------------------------------------------------------------------------------------------- embeddings
def int_valued(shape, seed, step=2.0 ** -3, lo=-8, hi=8):
    """fp32 values step * j, j uniform in lo .. hi (integers), step a power of two: a sum of n of them is exact in fp32, in any order, while n * max(|lo|, |hi|) < 2**24"""
    assert step > 0 and float(np.log2(step)).is_integer()
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32) * float(step)


def embed_bwd_ref(ids, dx, V, *, scale=1.0, pos_offset=0, n_pos=None, dwte0=None, dwpe0=None):
    """ids (..., U) int64, dx (M, d) -> (dwte (V, d), dwpe (n_pos, d) or None) fp64, added to dwte0 / dwpe0 (the op accumulates).  ids outside [0, V) add nothing."""
    ids = ids.detach().cpu().long()
    U = ids.shape[-1]
    flat = ids.reshape(-1)
    M = flat.numel()
    dx = dx.detach().cpu().to(F64)
    d = dx.shape[1]
    dwte = torch.zeros(V, d, dtype=F64) if dwte0 is None else dwte0.detach().cpu().to(F64).clone()
    ok = (flat >= 0) & (flat < V)
    dwte.index_add_(0, flat[ok], scale * dx[ok])
    dwpe = None
    if n_pos is not None:
        dwpe = torch.zeros(n_pos, d, dtype=F64) if dwpe0 is None else dwpe0.detach().cpu().to(F64).clone()
        dwpe.index_add_(0, pos_offset + torch.arange(M) % U, dx)
    return dwte, dwpe


def embed_fwd_ref(ids, wte, pos, *, scale=1.0, pos_offset=0, U=None):
    """(M, d) fp64 = scale * wte[clamp(ids, 0, V - 1)] + pos[pos_offset + m % U]"""
    ids = ids.detach().cpu().long()
    U = ids.shape[-1] if U is None else U
    flat = ids.reshape(-1).clamp(0, wte.shape[0] - 1)
    M = flat.numel()
    return scale * wte.detach().cpu().to(F64)[flat] + pos.detach().cpu().to(F64)[pos_offset + torch.arange(M) % U]


def exact(got, want_f64):
    """every element of the fp32 device result is the fp64 reference value, bit for bit once widened (NaN never is)"""
    return torch.equal(got.detach().cpu().to(F64), want_f64)


# ---------------------------------------------------------------------------------------------------------------- optimizer
def adamw_ref(p, g, m, v, decay=None, *, lr, betas, eps, weight_decay, step, coef=1.0, skip=False):
    """torch.optim.AdamW (decoupled decay) in fp64 on the fp32 inputs -> (p, m, v) fp64.  decay: boolean mask of the elements that decay (None: all);
    coef: the clip coefficient the gradient is multiplied by; skip: the step is dropped and everything comes back unchanged."""
    p, g, m, v = (t.detach().cpu().to(F64).clone() for t in (p, g, m, v))
    if skip:
        return p, m, v
    b1, b2 = betas
    g = g * coef
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    dec = torch.ones_like(p, dtype=torch.bool) if decay is None else decay.detach().cpu().bool()
    p = torch.where(dec, p * (1.0 - lr * weight_decay), p)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v


def clip_ref(sumsq, max_norm, skip_above=0.0):
    """[norm, coef, skip] of torch.nn.utils.clip_grad_norm_ plus the drop-the-step rule: coef = min(1, max_norm / (norm + 1e-6)) when max_norm > 0;
    skip (and coef = 0) when the norm is not finite or above skip_above > 0"""
    norm = float(np.sqrt(np.float64(sumsq))) if sumsq == sumsq and sumsq >= 0 else float("nan")
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    skip = (not np.isfinite(norm)) or (skip_above > 0 and norm > skip_above)
    return [norm, 0.0 if skip else coef, 1.0 if skip else 0.0]
