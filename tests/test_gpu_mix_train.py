"""GPU: mixing fine-tuning of the DeCRED decoder (modes `linear` and `scalar`) — the kernel pair mi_mix_ce (csrc/mix_loss.hip) against an fp64 restatement fed the same
fp32 per-head logits, and the model's training-mode forward (frozen body on the trainer's forward stages, `d lm_mixing` through a small autograd.Function) against the
reference fixture tests/golden/gen_tiny_mix.npz at B = 1 and the fp64 restatement tests/mix_ref.py at B = 3, then AdamW steps on `lm_mixing` alone."""
import pytest
import torch
import torch.nn.functional as F

import gen_model as GM
import mix_ref as MR
from helpers import AED_JCFG, compare_grads, load_golden, synth_feats
from huggingface_asr_amd import ops_train as T
from huggingface_asr_amd import shapes
from oracle import aed_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
ROWS, COLS = 64, 256                     # csrc/mix_loss.hip MIX_ROWS (rows per chunk of the gradient's reduction), MIX_COLS (columns per block)


def _kernel_case(B, U, V, H, per_col, seed):
    g = torch.Generator().manual_seed(seed)
    ld = T.pad64(V)
    lg = torch.full((H, B, U, ld), 1e30)                             # the padding columns hold a value that would wreck a log-sum-exp that read them
    lg[..., :V] = torch.randn(H, B, U, V, generator=g) * 3.0
    mix = 0.5 + 0.3 * torch.randn((H, V) if per_col else (H,), generator=g)
    lab = torch.randint(0, V, (B, U), generator=g)
    lab[torch.rand(B, U, generator=g) < 0.2] = -100                  # ignored rows
    lab[0, 1] = V - 1                                                # a label at the last column
    if B > 1:
        lab[1] = -100                                                # an utterance entirely ignored
    return lg, mix, lab


@pytest.mark.parametrize("per_col", [True, False], ids=["linear", "scalar"])
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("V", [51, COLS + 44])
@pytest.mark.parametrize("B,U", [(5, 13), (1, 2 * ROWS + 3)])
def test_mix_ce_against_fp64(B, U, V, H, per_col):
    """V = 51 (a row stride of 64) and V = 300 (two column tiles of the gradient kernel, the second ragged); M = B U = one row chunk + 1 and two chunks + 3; rows with
    -100, one utterance entirely ignored, a label at column V - 1.  Loss at the tolerance tests/test_gpu_train_ops.py holds `ce_label_smoothing` to (1e-4 absolute and
    relative).  Gradient: that file's elementwise bound for the cross-entropy gradient (tests/train_tail_ref.py `ce_grad_tol`: 2^-8 of the value + 2^-16 of the sum of
    the magnitudes of the terms that cancel), carried through dmix[h, v] = sum_r dz[r, v] L_h[r, v]: 2^-8 |want| + 2^-16 sum_r (p + onehot) |L_h| / N (scalar mode: summed
    over v as well).  Two runs give the same bits."""
    assert B * U in (ROWS + 1, 2 * ROWS + 3)
    lg, mix, lab = _kernel_case(B, U, V, H, per_col, seed=B * 1000 + V + H)
    m64 = mix.double().requires_grad_(True)
    L64 = lg[..., :V].double()
    z = (L64 * (m64[:, None, None, :] if per_col else m64[:, None, None, None])).sum(0)
    tgt = lab[:, 1:].reshape(-1)
    want = F.cross_entropy(z[:, :-1].reshape(-1, V), tgt, ignore_index=-100)
    want.backward()
    lgd, mixd, labd = lg.to(DEV), mix.to(DEV), lab.to(DEV)
    acc, lse = T.mix_ce_fwd(lgd, mixd, labd, V)
    loss = (acc[0] / acc[1]).cpu()
    n = int((tgt >= 0).sum())
    assert float(acc[1]) == n
    print(f"B={B} U={U} V={V} H={H} per_col={per_col}: loss {float(loss):.6f} vs {float(want):.6f}")
    torch.testing.assert_close(loss.double(), want.detach(), atol=1e-4, rtol=1e-4)
    dmix = T.mix_ce_bwd(lgd, mixd, labd, V, acc, lse)
    # the bound, term by term
    p = torch.softmax(z.detach()[:, :-1].reshape(-1, V), -1)
    valid = tgt >= 0
    onehot = torch.zeros_like(p)
    onehot[valid, tgt[valid]] = 1.0
    mag = ((p + onehot) * valid[:, None])[None] * L64[:, :, :-1].reshape(H, -1, V).abs() / n          # (H, rows, V)
    tol = 2.0 ** -16 * mag.sum(1)
    tol = tol if per_col else tol.sum(1)
    tol = 2.0 ** -8 * m64.grad.abs() + tol + 2.0 ** -126
    err = (dmix.cpu().double() - m64.grad).abs()
    print(f"    dmix worst err / tol {float((err / tol).max()):.4f}")
    assert dmix.shape == mix.shape and bool((err <= tol).all()), float((err / tol).max())
    acc2, lse2 = T.mix_ce_fwd(lgd, mixd, labd, V)
    assert torch.equal(acc, acc2) and torch.equal(lse, lse2) and torch.equal(dmix, T.mix_ce_bwd(lgd, mixd, labd, V, acc2, lse2))


NO_DROPOUT = dict(hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, final_dropout=0.0, feat_proj_dropout=0.0, csgu_conv_dropout=0.0,
                  apply_spec_augment=False, layerdrop=0.0)


def _mixing_model(mode, sd):
    from test_mix_cpu import _swap
    from test_surface_cpu import _joint_model
    model = _joint_model(False)
    for k, v in NO_DROPOUT.items():
        setattr(model.config.encoder, k, v)
    for k in ("resid_pdrop", "embd_pdrop", "attn_pdrop"):
        setattr(model.config.decoder, k, 0.0)
    model = _swap(model, mode)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return model.to(DEV).train()


def _restated(sd, dec_cfg, x, am, lab):
    """the restatement with the head products, the mix and the cross-entropy in fp64 (the oracle's body is fp32) -> (losses, d dec_loss / d lm_mixing)"""
    leaf = {k: (v.double() if "lm_mixing" in k else v).clone().requires_grad_("lm_mixing" in k) for k, v in sd.items()}
    with MR.patched(torch.float64):
        out = A.joint_forward(leaf, ENC, dec_cfg, AED_JCFG, x, am, lab)
    out["dec_loss"].backward()
    return out, leaf["decoder.lm_mixing"].grad


@pytest.mark.parametrize("mode", ["linear", "scalar"])
def test_model_training_forward_against_the_reference_and_the_restatement(mode):
    """all dropouts 0.  B = 1: `dec_loss`, `loss` and `d lm_mixing` against the reference's own numbers (gen_tiny_mix.npz) — losses at the 2e-3 relative of
    tests/test_gpu_aed.py, the gradient by `helpers.compare_grads` (relative L2 error 0.03, cosine 0.999: the bound every gradient of the training step is held to).
    B = 3 with ragged labels: the same against the fp64 restatement (the reference is undefined there)."""
    torch.set_num_threads(8)
    g = load_golden("gen_tiny_mix")
    sd, x, am, dec_cfg = MR.mix_case_inputs(mode)
    model = _mixing_model(mode, sd)
    n = int(am[0].sum())
    lab1 = torch.from_numpy(g["labels"])
    out = model(input_values=x[:1, :n].to(DEV), attention_mask=am[:1, :n].to(DEV), labels=lab1.to(DEV))
    for k in ("loss", "enc_loss", "dec_loss"):
        print(mode, "B = 1", k, float(getattr(out, k)), float(g[f"{mode}/{k}"]))
        assert abs(float(getattr(out, k)) - float(g[f"{mode}/{k}"])) < 2e-3 * abs(float(g[f"{mode}/{k}"])), k
    out.dec_loss.backward()
    grads = {n_: p.grad for n_, p in model.named_parameters() if p.grad is not None}
    assert sorted(grads) == ["decoder.lm_mixing"]
    print(mode, "B = 1 dmix", compare_grads({"m": grads["decoder.lm_mixing"]}, {"m": g[f"{mode}/dmix"]}))
    # B = 3, ragged labels
    seed = GM.CASES["gen_tiny"][0]
    x3, am3 = synth_feats(seed, 3, 200, [198, 131, 160])
    lab3 = torch.tensor([[5, 17, 30, 9, 22, 41, 12, 1], [8, 40, 3, 1, -100, -100, -100, -100], [11, 1, -100, -100, -100, -100, -100, -100]])
    model.zero_grad(set_to_none=True)
    out = model(input_values=x3.to(DEV), attention_mask=am3.to(DEV), labels=lab3.to(DEV))
    want, dwant = _restated(sd, dec_cfg, x3, am3, lab3)
    for k in ("loss", "enc_loss", "dec_loss"):
        print(mode, "B = 3", k, float(getattr(out, k)), float(want[k]))
        assert abs(float(getattr(out, k)) - float(want[k])) < 2e-3 * abs(float(want[k])), k
    out.loss.backward()                                             # through loss = w enc_loss + (1 - w) dec_loss: d lm_mixing = (1 - w) d dec_loss
    got = model.decoder.lm_mixing.grad / (1 - AED_JCFG["ctc_weight"])
    print(mode, "B = 3 dmix", compare_grads({"m": got}, {"m": dwant.float()}))


def test_adamw_steps_on_the_mix_lower_the_loss_and_leave_the_rest():
    """5 AdamW steps (torch's optimizer, as HF `Trainer` runs it) on `lm_mixing`: the loss falls, every other parameter keeps its bits, and the evaluation engine
    decodes with the updated mix"""
    sd, x, am, dec_cfg = MR.mix_case_inputs("linear")
    model = _mixing_model("linear", sd)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=0.05)
    lab = torch.tensor([[5, 17, 30, 9, 22, 41, 12, 1], [8, 40, 3, 1, -100, -100, -100, -100]]).to(DEV)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        out = model(input_values=x.to(DEV), attention_mask=am.to(DEV), labels=lab)
        out.loss.backward()
        opt.step()
        losses.append(float(out.loss))
    print("losses", losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v) == ("lm_mixing" not in k), k
    model.eval()
    with torch.no_grad():
        ev = model(input_values=x.to(DEV), attention_mask=am.to(DEV), labels=lab)
    assert float(ev.loss) < losses[0]


def test_what_mixing_fine_tuning_refuses():
    sd, x, am, dec_cfg = MR.mix_case_inputs("linear")
    model = _mixing_model("linear", sd)
    lab = torch.tensor([[5, 17, 30, 1]]).to(DEV)
    next(model.encoder.parameters()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="model_utils.py:214-217"):
        model(input_values=x[:1].to(DEV), attention_mask=am[:1].to(DEV), labels=lab)
    sdf, _, _, _ = MR.mix_case_inputs("full")
    full = _mixing_model("full", sdf)
    with pytest.raises(NotImplementedError, match="`full` mixing mode"):
        full(input_values=x[:1].to(DEV), attention_mask=am[:1].to(DEV), labels=lab)
    with torch.no_grad():                                            # evaluation with labels runs for every mode
        assert torch.isfinite(full.eval()(input_values=x[:1].to(DEV), attention_mask=am[:1].to(DEV), labels=lab).loss)
