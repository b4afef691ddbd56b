"""CPU proof that the zero tolerance of tests/test_gpu_attention_probes.py is legitimate, and that its case tables reach every edge the probes are there for
(tests/attention_cases.py).  No GPU."""
import math

import pytest
import torch

import attention_cases as AC

SMALL = [c for c in AC.ALL if c.B <= 100]            # the two block-id cases of 65 k blocks are gathers of 3 x 3 score matrices: checked apart, without the emulation
SELECTOR = [c for c in SMALL if c.family != "D"]
FAMILY_D = [c for c in AC.ALL if c.family == "D"]


def _row_mask(case, exact):
    return exact.permute(0, 2, 1).unsqueeze(-1).expand(case.B, case.Tq, case.H, case.hd).reshape(case.B, case.Tq, -1)


def test_operands_are_bf16_exact_and_v_has_no_zero():
    for c in AC.ALL:
        inp = AC.build(c)                             # build() asserts bf16 exactness of every operand and of q + bias
        for name in ("q", "k", "v"):
            assert AC.bf16_exact(inp[name]), (c.name, name)
        if c.family != "D":
            assert bool((inp["v"] != 0).all()) and bool(inp["v"].abs().max() <= 126), c.name
            assert inp["k"].shape[1] == (c.Lmax or c.Tk) and inp["v"].shape[1] == (c.Lmax or c.Tk), c.name


def test_winners_are_unique_by_20_nats_in_fp64():
    for c in [c for c in AC.ALL if c.family != "D"]:
        inp = AC.build(c)
        _, _, s = AC.reference(c, inp)
        w = inp["winner"]
        ex = w >= 0
        assert bool((AC.selected(c, inp) == w)[ex].all()), c.name
        top = torch.gather(s, 3, w.clamp(min=0).unsqueeze(-1))
        rest = s.scatter(3, w.clamp(min=0).unsqueeze(-1), -math.inf).max(-1).values
        gap = (top.squeeze(-1) - rest)[ex]
        assert bool((gap >= AC.GAP_NATS).all()), (c.name, float(gap.min()))
        if c.family != "C":
            assert bool(ex.all()), c.name             # families A, A', B check every row exactly


def test_selector_cases_exact_under_every_honest_emulation():
    for c in SELECTOR:
        inp = AC.build(c)
        want, ex = AC.expected_rows(c, inp)
        m = _row_mask(c, ex)
        for kw in AC.EMU_VARIANTS:
            out, _ = AC.emulate(c, inp, **kw)
            assert torch.equal(out[m], want[m]), (c.name, kw, int((out[m] != want[m]).sum()))
            assert bool(torch.isfinite(out).all()), (c.name, kw)


def test_family_a_lse_is_the_winners_score():
    """what the GPU test asserts on one family A case per lse entry: with the leak <= Tk e^-20 the row's log-sum-exp is the winner's scaled score."""
    for c in [c for c in SMALL if c.family in ("A", "A1") and c.entry in ("qkv_lse", "xlse")]:
        inp = AC.build(c)
        _, lse2, s = AC.reference(c, inp)
        top = torch.gather(s, 3, inp["winner"].unsqueeze(-1)).squeeze(-1) * AC.LOG2E
        assert float((lse2 - top).abs().max()) < 1e-6, c.name


def _caught(c, inp, **mut):
    ex = inp["winner"] >= 0
    return bool((AC.selected(c, inp, **mut) != inp["winner"])[ex].any())


def _fraction_changed(c, inp, **mut):
    ex = inp["winner"] >= 0
    return float((AC.selected(c, inp, **mut) != inp["winner"])[ex].float().mean())


def test_mutants_change_an_exact_row_of_every_case_they_reach():
    n = dict(len_minus=0, len_plus=0, diag_minus=0, diag_plus=0, shift=0)
    for c in SELECTOR:
        inp = AC.build(c)
        lens = AC.eff_lengths(c)
        coff = c.Tk - c.Tq
        if c.family in ("A", "A1"):
            # the last visible key is the winner: dropping it (len - 1) reaches every case whose last row sees key len - 1
            if any(c.Tq - 1 + coff >= n_ - 1 for n_ in lens) or not c.causal:
                assert _caught(c, inp, dlen=-1), ("len - 1", c.name)
                n["len_minus"] += 1
            # one key too many reaches a batch with a key past its length that some row may see
            if any(n_ < c.Tk and (not c.causal or c.Tq - 1 + coff >= n_) for n_ in lens):
                assert _caught(c, inp, dlen=1), ("len + 1", c.name)
                n["len_plus"] += 1
            if c.causal:
                assert _caught(c, inp, ddiag=-1), ("diagonal - 1", c.name)
                n["diag_minus"] += 1
                if any(i + coff + 1 < n_ for n_ in lens for i in (0,)):
                    assert _caught(c, inp, ddiag=1), ("diagonal + 1", c.name)
                    n["diag_plus"] += 1
        if c.family == "B" and c.causal and c.Tk == c.Tq:
            assert _caught(c, inp, ddiag=-1), ("diagonal - 1", c.name)       # the rows whose target is clipped to the diagonal
        if c.family == "C":          # (family A' is a monotone ramp over the relative position: shifted by one it still ends on the last key)
            for ds in (1, -1):
                assert _caught(c, inp, dshift=ds), ("shift", ds, c.name)
                assert _fraction_changed(c, inp, dshift=ds) >= 0.5, c.name        # (measured: 0.79 at T = 50 causal, >= 0.9 elsewhere)
            n["shift"] += 1
    assert all(v > 10 for v in n.values()), n


def test_batch_base_mutant_changes_every_strided_case():
    """family A: every strided case.  Family B looks a key up by its bits, and row b * Tk + j of the flat cache is a real (batch, key) row whose V row is the right one whenever
    it is found at all — a single-row step with a small target is blind to this mutant, so there only most cases are required to change."""
    strided = [c for c in AC.ALL if c.Lmax]
    assert len(strided) >= 80
    caught_b = []
    for c in strided:
        inp = AC.build(c)
        want, _ = AC.expected_rows(c, inp)
        got, _, _ = AC.reference(c, inp, kv=AC.batch_base_mutant(c, inp))
        changed = bool((got.float() != want).any())
        assert c.Lmax > c.Tk
        if c.family == "A":
            assert changed, c.name
        else:
            caught_b.append(changed)
    assert sum(caught_b) >= 0.75 * len(caught_b), (sum(caught_b), len(caught_b))


def test_family_c_checks_40_percent_of_its_rows_exactly():
    cs = [c for c in AC.ALL if c.family == "C"]
    assert cs
    for c in cs:
        ex = AC.build(c)["winner"] >= 0
        assert float(ex.float().mean()) >= AC.C_MIN_EXACT, (c.name, float(ex.float().mean()))
        for h in range(c.H):                      # and no head (offset) goes unchecked
            assert bool(ex[:, h].any()), (c.name, c.deltas[h])


def _d_worst():
    worst, worst_lse, who = 0.0, 0.0, None
    for c in FAMILY_D:
        inp = AC.build(c)
        want, lse2, _ = AC.reference(c, inp)
        for kw in AC.EMU_VARIANTS:
            out, lse = AC.emulate(c, inp, **kw)
            e = float(AC.d_normalised_error(out, want).max())
            if e > worst:
                worst, who = e, (c.name, kw)
            worst_lse = max(worst_lse, float((lse.double() - lse2).abs().max()))
    return worst, worst_lse, who


def test_family_d_constant():
    worst, worst_lse, who = _d_worst()
    print(f"family D: worst normalised error of the emulation {worst:.3f} at {who}; worst |lse| error {worst_lse:.2e}")
    assert abs(AC.D_C / (3 * worst) - 1) <= 0.10, (worst, who)
    assert worst_lse < AC.LSE_TOL / 10
    # the tied rows of family C are held to the same bound
    for c in [c for c in AC.ALL if c.family == "C"]:
        inp = AC.build(c)
        want, _, _ = AC.reference(c, inp)
        for kw in AC.EMU_VARIANTS:
            out, _ = AC.emulate(c, inp, **kw)
            assert float(AC.d_normalised_error(out, want).max()) <= AC.D_C, (c.name, kw)


def test_family_d_ramps_exercise_the_lazy_rescale():
    """the profiles do what their names say: per 32-key tile the row maximum moves by 32 rho in the exp2 domain."""
    for c in FAMILY_D:
        if c.prof == "jump" or c.causal or c.rel:
            continue
        _, _, s = AC.reference(c, AC.build(c))
        n = AC.eff_lengths(c)[0]
        if n < 96:
            continue
        tmax = torch.stack([s[0, :, :, 32 * t:32 * t + 32].max(-1).values for t in range(n // 32)], -1) * AC.LOG2E
        step = float((tmax[..., 1:] - tmax[..., :-1]).mean())
        assert abs(step - 32 * c.prof) < 1.0, (c.name, step)
    assert 32 * 0.34 < AC.RESCALE_THRESHOLD < 32 * 0.36


def test_reciprocal_quotient_exact_below_2_16_and_not_beyond():
    ids = torch.arange(1 << 16, dtype=torch.int64).view(1, -1)
    wrong_beyond = 0
    for g0 in range(2, 513, 73):
        g = torch.arange(g0, min(g0 + 73, 513), dtype=torch.int64).view(-1, 1)
        m = ((1 << 32) + g - 1) // g
        assert torch.equal((ids * m) >> 32, ids // g), g0
    for g in (1, 2, 3, 5, 15, 511, 512):
        assert AC.recip_quotient(65535, g) == 65535 // g
    # exact while id * g < 2^32; past 2^16 ids the quotient by a divisor the launcher could see is wrong
    for g, i in ((65535, 131069), (511, 8967027)):
        wrong_beyond += AC.recip_quotient(i, g) != i // g
        assert AC.recip_quotient(i - 1, g) == (i - 1) // g
    assert wrong_beyond > 0                                  # the launcher's bound is real
    # the block order is a permutation onto every (query block, head, batch)
    for gx, H, B in ((1, 15, 4369), (3, 5, 7), (2, 8, 4), (3, 2, 3)):
        N = gx * H * B
        seen = {AC.block_decode(L, N, gx, H) for L in range(N)}
        assert seen == {(x, h, b) for x in range(gx) for h in range(H) for b in range(B)}, (gx, H, B)


def test_block_id_cases_sit_on_the_limit():
    a, b, c = AC.BLOCKID
    assert AC.nblocks(a) == 65535 and AC.forms_of(a) == ["lds8", "lds8"]
    assert AC.nblocks(b) == 65550 and AC.forms_of(b) == ["lds4"]
    assert -(-c.Tq // 128) == 3 and c.H == 5 and "lds8" in AC.forms_of(c)
    for case in (a, b):
        inp = AC.build(case)
        assert bool((AC.selected(case, inp) == inp["winner"]).all())


def test_case_tables_reach_every_combination():
    have = set()
    for c in AC.ALL:
        for form in AC.forms_of(c):
            have.add((c.entry, form, c.hd, c.rel, c.causal, "D" if c.family == "D" else "selector"))
    need = set()
    for kind in ("selector", "D"):
        for rel in (False, True):
            for causal in (False, True):
                for hd in (16, 32, 64, 128):
                    need.add(("reg", "reg", hd, rel, causal, kind))
                for hd in (64, 128):
                    need.add(("qkv", "lds4", hd, rel, causal, kind))
                    need.add(("qkv", "lds8", hd, rel, causal, kind))
                    need.add(("qkv_lse", "lds4" if (hd == 64 and rel) else "lds8", hd, rel, causal, kind))
        for hd in (64, 128):
            for form in ("lds4", "lds8"):
                need.add(("general", form, hd, False, False, kind))
            need.add(("general", "lds4", hd, False, True, "selector"))
            need.add(("general", "lds8", hd, False, True, "selector"))
            need.add(("xlse", "lds8", hd, False, False, kind))
            need.add(("xlse", "lds8", hd, False, True, kind))
    missing = sorted(map(str, need - have))
    assert not missing, missing
    # the edges each table is there for, by name
    sq = [c for c in AC.SQUARE if c.group == "square"]
    for entry in ("reg", "qkv", "qkv_lse"):
        assert {c.Tq for c in sq if c.entry == entry} >= set(AC.SQUARE_T), entry
    assert any(1 in c.lengths and c.Tq + 5 in c.lengths for c in sq)
    for fam in ("A", "A1", "B", "C", "D"):
        assert any(c.family == fam for c in sq), fam
    assert any(c.family == "C" and c.Tq == 50 for c in AC.SQUARE)
    for form in ("lds4", "lds8"):
        for hd in (64, 128):
            profs = {c.prof for c in FAMILY_D if c.hd == hd and form in AC.forms_of(c) and c.Tk >= 250}
            assert profs == set(AC.D_PROFILES), (form, hd, profs)
    step = [c for c in AC.CACHE if c.group == "step"]
    assert {c.Tk - 1 for c in step} == {0, 30, 31, 32, 127, 128, 255, 256} and {c.B for c in step} == {3, 10}
    assert all(c.Tq == 1 and c.Lmax == AC.LMAX and c.H == 2 and c.causal and c.variants == (0, 1, 2) for c in step)
    for past in (0, 30, 31, 32, 127, 128, 255, 256):
        assert {(c.B, c.hd, c.family) for c in step if c.Tk == past + 1} == {(B, hd, f) for B in (3, 10) for hd in (64, 128) for f in "AB"}
    chunk = [c for c in AC.CACHE if c.group == "chunk"]
    assert {(c.Tq, c.Tk - c.Tq, c.hd) for c in chunk} == {(U, p, hd) for U in (5, 33, 129, 160) for p in (0, 31, 100) for hd in (64, 128)}
    assert {c.family for c in chunk if c.Tq > 128 and c.Tk > c.Tq} == {"A", "B"}       # a second query block under a non-zero causal offset
    assert all(c.Tk <= c.Lmax for c in AC.CACHE)
    cross = [c for c in AC.CROSS if c.group == "cross"]
    for entry in ("general", "xlse"):
        assert {(c.Tq, c.Tk, c.hd) for c in cross if c.entry == entry} == {(q, k, hd) for q in (1, 7, 130) for k in (33, 250, 500) for hd in (64, 128)}
        for Tk in (33, 250, 500):
            ls = set().union(*[set(c.lengths) for c in cross if c.entry == entry and c.Tk == Tk])
            assert ls >= {1, 31, 32, 33, Tk - 1, Tk, Tk + 5}, (entry, Tk, ls)
    assert {(c.Tq, c.hd) for c in AC.CROSS if c.group == "xcausal"} == {(T, hd) for T in (33, 130) for hd in (64, 128)}
    # rel hd = 64 runs on both LDS-staged forms (the product routes it to the four-wave kernel)
    assert any(c.rel and c.hd == 64 and set(AC.forms_of(c)) == {"lds4", "lds8"} for c in sq)
