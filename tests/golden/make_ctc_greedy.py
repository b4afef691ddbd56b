"""Generator of tests/golden/ctc_greedy.npz: seeded logits and what the REFERENCE's ctc_greedy_decode returns for them.

    python tests/golden/make_ctc_greedy.py <path to the reference's src/utilities/eval_utils.py>

The reference module cannot be imported where its third-party imports (jiwer, torchaudio, wandb) are absent, so the one function is taken out of the file's
syntax tree at generation time and run with only `torch` and `itertools` in scope.  Only data is stored: the logits, (blank, pad) and the returned ids."""
import ast
import itertools
import os
import sys

import numpy as np
import torch

V1 = 51


def reference_function(path):
    tree = ast.parse(open(path).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "ctc_greedy_decode")
    scope = {"torch": torch, "it": itertools, "itertools": itertools}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), scope)
    return scope["ctc_greedy_decode"]


def cases():
    """name -> (logits (B, T, V1), blank, pad).  The logits are multiples of 1/8 in [-16, 16) — stored as int8, exact in fp32 and in bf16 — so equal maxima occur in
    every case, not only in the one built for them."""
    g = torch.Generator().manual_seed(20240607)
    rnd = lambda *s: torch.clamp(torch.round(torch.randn(*s, generator=g) * 16.0), -100, 100)          # in eighths
    out = {}
    out["random"] = (rnd(2, 10, V1), V1 - 1, 0)
    x = rnd(2, 10, V1); x[..., V1 - 1] += 40
    out["blank_dominated"] = (x, V1 - 1, 3)
    x = rnd(2, 10, V1); x[1, :, V1 - 1] = 120
    out["all_blank_row"] = (x, V1 - 1, 1)
    x = rnd(2, 10, V1); x[0, :, 17] = 120
    out["single_token_row"] = (x, V1 - 1, 0)
    x = rnd(2, 16, V1); x[:, ::3, 7] += 60; x[:, 1::5, 12] += 80; x[..., 30] = x[..., 7]; x[..., V1 - 1] = x[..., 12]
    out["exact_ties"] = (x, V1 - 1, 2)
    x = rnd(2, 10, V1); x[..., 5] += 40
    out["blank_not_last"] = (x, 5, 50)
    return {k: (torch.clamp(x, -128, 127) / 8.0, b, p) for k, (x, b, p) in out.items()}


def main():
    ref = reference_function(sys.argv[1])
    data, meta = {}, []
    for name, (x, blank, pad) in sorted(cases().items()):
        ids = ref(x.clone(), blank, pad)
        data[name + ".q8"] = (x * 8.0).numpy().astype(np.int8)           # logits = q8 / 8
        data[name + ".ids"] = ids.numpy().astype(np.int8)
        meta.append((blank, pad))
    data["meta"] = np.asarray(meta, dtype=np.int8)                       # (blank, pad) per case, cases in sorted order
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ctc_greedy.npz"), **data)


if __name__ == "__main__":
    main()
