"""Cases and exact references for the two GEMM families of the backward pass — the weight-gradient GEMM (huggingface_asr_amd/csrc/gemm_tn.hip: mi_gemm_tn_bf16,
mi_conv2d_wgrad_cl_bf16, mi_gemm_tn_group_ow_bf16) and the strided batched GEMM of the materialising attention backward (huggingface_asr_amd/csrc/bgemm.hip:
mi_bgemm_sparse_bf16) — shared by tests/test_tn_cases_cpu.py (no GPU) and tests/test_gpu_tn_forms.py.  Nothing here touches a GPU.

Exact inputs.  Weight gradient: dY and X are integers drawn from {+-1, +-2, +-3} — no zeros, so a dropped or doubled row moves EVERY element of dW and of db — and
the dW / db a launch adds into hold integers in {-8..8}.  With M <= 70 000 rows every partial sum has magnitude <= 9 M < 2**24 (twice that after the second adding
call, still below), so the fp32 accumulation order, the number of M splits, the order in which the slab reduce adds them and the `v_dot2_f32_bf16` column sums of
the bias gradient all give the same, exactly representable value: float64 `base + dY[:, :n_store].T @ X` and `base + dY.sum(0)[:n_store]`.
bgemm: A and B are integers in {-3..3}, K <= 4096, alpha in {1, 0.5}, the C an accumulating launch adds into holds integers in {-8..8}: the fp32 output is the
float64 value bit for bit, the bf16 output its round-to-nearest-even cast (`f2bf`, huggingface_asr_amd/csrc/common.hpp) — in accumulate mode the cast of
fp32(alpha * acc) + C, which is exact before the cast.  Every tolerance is zero.

Poison.  What a kernel may read but must not use holds NaN (columns beside an operand view, row padding, buffer rows below M, whole dead tiles), and so does
everything it must not write.  The one exception is data the contract calls zero and multiplies anyway: the band operand outside its band and the A rows at or
past `m_valid` inside a live tile are true zeros.

THE WEAK POINT.  Neither family takes a profiling slot, so WHICH kernel a case reaches cannot be observed: every case's `form` is derived with the Python copies
below of tn_splits, tn_big, the rows_per_split rule, the `fast_ok` condition of tn_tile, the grouped launch's tile choice, and bgemm's bg_operand_fast and tile
choice.  If gemm_tn.hip or bgemm.hip change one of them, change the copy with it; tests/test_tn_cases_cpu.py pins each at its thresholds.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

TN_KM = 64                                   # rows (m) per LDS stage
M_BOUND = 70000                              # 2 * 9 * M + 8 < 2**24
FAST_LIMIT = 2 ** 32 - 4096                  # tn_tile: the buffer-descriptor loader needs M * max(ldy, ldx) * 2 below this
TN_GROUP = 48
ARG, UNSUPPORTED = -1, -3                    # MI_ERR_ARG, MI_ERR_UNSUPPORTED


def cdiv(a, b):
    return (a + b - 1) // b


def rup(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------------------------------------------------------------------
# Python copies of the dispatch (see THE WEAK POINT)
def tn_splits(M, N, K, variant):
    """gemm_tn.hip tn_splits; variant 2 = the 256 x 256 tile"""
    xw = 64 if variant == 1 else 128
    tiles = cdiv(N, 256) * cdiv(K, 256) if variant == 2 else cdiv(N, 128) * cdiv(K, xw)
    s = (256 if variant == 2 else 768 if variant == 1 else 512) // tiles
    s = min(s, cdiv(M, 4 * TN_KM))
    return max(s, 1)


def tn_big(M, N, K):
    return M >= 32768 and N >= 256 and K >= 256


def rows_per_split(M, splits):
    return cdiv(cdiv(M, splits), TN_KM) * TN_KM


def fast_ok(M, ldy, ldx, conv=False, gathered_big=False):
    """tn_tile: FAST (compiled out of the gathered 256 x 256 form) && !conv && the 32-bit range of a buffer descriptor"""
    return (not gathered_big) and (not conv) and M * max(ldy, ldx) * 2 < FAST_LIMIT


def group_xw(tile_k, problems):
    """mi_gemm_tn_group_ow_bf16: the k extent of the 256-row tiles; problems = [(M, N, K), ...]"""
    t256 = sum(cdiv(N, 256) * cdiv(K, 256) for _, N, K in problems)
    return tile_k if tile_k else (256 if t256 >= 200 else 128)


def group_permute(bid, nwg):
    """gemm_tn_group_kernel: hardware block id -> position in the tile list (consecutive ids go round-robin over 8 XCDs, each works through one contiguous run)"""
    q, r, xcd, idx = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def bg_operand_fast(base_elems, z1, z2, s_row, s_k, R, K):
    """bgemm.hip bg_operand_fast; base_elems = the operand's offset from a 16-B aligned address, in bf16 elements"""
    outer = s_row if s_k == 1 else s_k
    extent = K if s_k == 1 else R
    if (base_elems * 2) % 16 or z1 % 8 or z2 % 8 or outer % 8 or outer < 0:
        return False
    return extent % 8 == 0 or outer >= rup(extent, 8)


def bg_blocks128(M, N, Z):
    return cdiv(M, 128) * cdiv(N, 128) * Z


def bg_tile(M, N, Z):
    """mi_bgemm_sparse_bf16: 128 x 128 x 64 when that still gives every CU a block, else 64 x 64 x 32"""
    return 128 if M > 64 and N > 64 and bg_blocks128(M, N, Z) >= 256 else 64


Plan = namedtuple("Plan", "form tile splits rps rows stages last_rows empty loader")


def tn_plan(M, N, K, variant, ldy, ldx, conv_cin=None):
    """what mi_gemm_tn_bf16 (conv_cin None) / mi_conv2d_wgrad_cl_bf16 launches: per split its rows, stages and the valid rows of its last stage"""
    conv = conv_cin is not None
    big = variant == 0 and tn_big(M, N, K) and (not conv or conv_cin % 256 == 0)
    splits = tn_splits(M, N, K, 2 if big else variant)
    rps = rows_per_split(M, splits)
    rows = tuple(min(M, (s + 1) * rps) - s * rps for s in range(splits))                       # <= 0: a split that receives no rows (nit <= 0)
    stages = tuple(cdiv(r, TN_KM) if r > 0 else 0 for r in rows)
    last_rows = tuple(r - (n - 1) * TN_KM if n else 0 for r, n in zip(rows, stages))
    tile = "big" if big else ("t128x64" if variant == 1 else "t128")
    loader = "gather" if conv else ("desc" if fast_ok(M, ldy, ldx) else "ptr")
    return Plan(f"{tile}-{loader}", tile, splits, rps, rows, stages, last_rows, any(r <= 0 for r in rows), loader)


# ----------------------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
# xwide: 0, or the row length of the UNINITIALISED buffer X is a column view of (the 4 GiB cases)
TnCase = namedtuple("TnCase", "id variant M N K n_store db views xwide")
TnLayout = namedtuple("TnLayout", "y_off ldy x_off ldx w_off ldo")

M_SINGLE = (1, 15, 16, 17, 63, 64, 65, 128, 129, 192, 193)            # one split (M <= 256): 1 ... 4 stages, every class of ragged last stage (a k-step is 16 rows)
M_SPLIT = (257, 513, 1025)                                            # 2, 3 and 5 splits; the last split of 1025 has ONE row
NK_EDGES = (8, 72, 128, 136, 264)                                     # a tile of 8 columns; ragged tiles; K straddling 64 and 128; three tiles
BIG_M = (32768, 32769, 32768 + 4 * 64 * 3 + 17)
BIG_NK = ((256, 256), (264, 520), (512, 256))
HUGE_LD = 65544


def tn_layout(c) -> TnLayout:
    """views: dY = buf[:, 8:8+N] and X = buf[:, 16:16+K] inside wider NaN rows, dW = buf[:n_store, 4:4+K] with ldo > K.  Else contiguous."""
    if c.xwide:
        return TnLayout(8, c.N + 24, 32768, c.xwide, 4, c.K + 12)
    if c.views:
        return TnLayout(8, c.N + 24, 16, c.K + 24, 4, c.K + 12)
    return TnLayout(0, c.N, 0, c.K, 0, c.K)


def tn_case_plan(c) -> Plan:
    lo = tn_layout(c)
    return tn_plan(c.M, c.N, c.K, c.variant, lo.ldy, lo.ldx)


def _tn(variant, M, N, K, ns, db, views, xwide=0):
    cid = f"v{variant}-{M}x{N}x{K}-ns{ns}" + ("-db" if db else "") + ("-views" if views else "") + ("-4GiB" if xwide else "")
    return TnCase(cid, variant, M, N, K, ns, bool(db), bool(views), xwide)


def _ns(kind, N):
    return (N, N - 5, 1)[kind % 3]


def _build_tn():
    cases = []
    for variant in (0, 1):
        for mi, M in enumerate(M_SINGLE + M_SPLIT):
            N, K = NK_EDGES[(mi + variant) % 5], NK_EDGES[(2 * mi + variant + 1) % 5]
            cases.append(_tn(variant, M, N, K, _ns(mi + variant, N), (mi // 2 + variant) % 2, (mi + variant) % 2))
    # a split that receives no rows: 8 splits of 320 rows, the last starts at 2240 > M
    cases.append(_tn(0, 2049, 1024, 1024, 1019, True, True))
    # the 256 x 256 tile split over M (variant 0, M >= 32768, N, K >= 256), and one row fewer: the 128 tile on the same operands
    for mi, M in enumerate(BIG_M + (32767,)):
        for ni, (N, K) in enumerate(BIG_NK):
            cases.append(_tn(0, M, N, K, N - 5, (mi + ni) % 2, (mi + ni + 1) % 2))
    # the per-lane pointer fallback (M * ldx * 2 >= 2**32 - 4096): on the 128 tile (N < 256) and on the big one
    cases.append(_tn(0, 32776, 128, 136, 123, True, True, xwide=HUGE_LD))
    cases.append(_tn(0, 32776, 256, 256, 251, True, True, xwide=HUGE_LD))
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


TN_CASES = _build_tn()
TN_BY_ID = {c.id: c for c in TN_CASES}


def _ints_nz(shape, g):
    """integers in {+-1, +-2, +-3}"""
    return (torch.randint(1, 4, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).double()


@functools.lru_cache(maxsize=2)
def _tn_operands(M, N, K):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    dy, x = _ints_nz((M, N), g), _ints_nz((M, K), g)
    bw = torch.randint(-8, 9, (N, K), generator=g).double()
    bb = torch.randint(-8, 9, (N,), generator=g).double()
    return dy, x, bw, bb, dy.t() @ x, dy.sum(0)


def tn_inputs(c):
    """(dY (M, N), X (M, K), dW base (n_store, K), db base (n_store,)) as float64"""
    dy, x, bw, bb, _, _ = _tn_operands(c.M, c.N, c.K)
    return dy, x, bw[:c.n_store], bb[:c.n_store]


def tn_reference(c, calls=1):
    """float64 (dW, db) after `calls` adding launches"""
    _, _, bw, bb, prod, col = _tn_operands(c.M, c.N, c.K)
    return bw[:c.n_store] + calls * prod[:c.n_store], bb[:c.n_store] + calls * col[:c.n_store]


def tn_reference_f32(dy, x, order, chunk=TN_KM):
    """dY^T X and the column sums accumulated in float32 over row chunks taken in `order`: what a kernel's stage loop, its M splits and the slab reduce do, in any order"""
    dy, x = dy.float(), x.float()
    acc = torch.zeros((dy.shape[1], x.shape[1]), dtype=torch.float32)
    col = torch.zeros(dy.shape[1], dtype=torch.float32)
    for i in order:
        acc = acc + dy[i * chunk:(i + 1) * chunk].t() @ x[i * chunk:(i + 1) * chunk]
        col = col + dy[i * chunk:(i + 1) * chunk].sum(0)
    return acc, col


# ----------------------------------------------------------------------------------------------------------------------------------------
# Conv2d weight gradient (the gathered loader).  Tin / Fin = what the windows need, minus `trail` rows / columns (the last window then runs past the input: zeros)
ConvCase = namedtuple("ConvCase", "id B Tout Fout Cin Cout KH KW stride pad_t pad_f trail n_store db views")


def conv_dims(c):
    Tin = (c.Tout - 1) * c.stride + c.KH - c.pad_t - c.trail
    Fin = (c.Fout - 1) * c.stride + c.KW - c.pad_f - (c.trail if c.KW > 1 else 0)
    assert Tin >= 1 and Fin >= 1, c.id
    return Tin, Fin


def conv_mnk(c):
    return c.B * c.Tout * c.Fout, c.Cout, c.KH * c.KW * c.Cin


def conv_ldy(c):
    return c.Cout + 24 if c.views else c.Cout


def conv_plan(c) -> Plan:
    M, N, K = conv_mnk(c)
    return tn_plan(M, N, K, 0, conv_ldy(c), c.Cin, conv_cin=c.Cin)


def _cv(B, Tout, Fout, Cin, Cout, k=(3, 3), pad=(1, 1), trail=0, ns=None, db=True, views=False):
    ns = Cout if ns is None else ns
    cid = f"{B}x{Tout}x{Fout}-c{Cin}-o{Cout}-k{k[0]}x{k[1]}-p{pad[0]}{pad[1]}" + (f"-t{trail}" if trail else "") + f"-ns{ns}" + ("-db" if db else "") + ("-views" if views else "")
    return ConvCase(cid, B, Tout, Fout, Cin, Cout, k[0], k[1], 2, pad[0], pad[1], trail, ns, bool(db), bool(views))


def _build_conv():
    cases = [
        # 128 tile: the carried (b, to, fo) position wraps more than once per 64-row stage (Fout 1, 7, 19), once (64) or not in every stage (70); pads 0, 1, 2 (causal)
        _cv(3, 50, 1, 128, 72, pad=(1, 1), ns=67),
        _cv(2, 30, 7, 256, 136, pad=(0, 0), db=False, views=True),
        _cv(3, 25, 19, 128, 264, pad=(2, 2), ns=259, views=True),
        _cv(2, 5, 64, 256, 8, pad=(1, 1), trail=1, ns=3),
        _cv(2, 4, 70, 128, 136, pad=(2, 2), db=False),
        _cv(3, 9, 19, 256, 72, pad=(1, 1), trail=1, views=True),
        # a time-only (3, 1) kernel
        _cv(2, 31, 7, 128, 72, k=(3, 1), pad=(1, 0), views=True),
        _cv(2, 12, 64, 256, 136, k=(3, 1), pad=(2, 0), ns=1),
        # B Tout Fout in {1, 63, 65, 257}
        _cv(1, 1, 1, 128, 8, pad=(1, 1)),
        _cv(1, 9, 7, 256, 72, pad=(2, 2), views=True),
        _cv(1, 5, 13, 128, 136, pad=(0, 0), ns=131),
        _cv(1, 257, 1, 128, 72, k=(3, 1), pad=(1, 0)),
        # the gathered 256 x 256 form (Cin % 256 == 0, Cout >= 256, B Tout Fout >= 32768) as a large batch of short inputs, one case exactly at 32768 rows ...
        _cv(64, 32, 17, 256, 256, pad=(1, 1), ns=251),
        _cv(64, 32, 16, 256, 264, k=(3, 1), pad=(2, 0), views=True),
        # ... and the same geometries at Cin = 128, where `big` is refused and the 128 tile runs
        _cv(64, 32, 17, 128, 256, pad=(1, 1), ns=251),
        _cv(64, 32, 16, 128, 264, k=(3, 1), pad=(2, 0), views=True),
    ]
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


CONV_CASES = _build_conv()


@functools.lru_cache(maxsize=2)
def conv_inputs(c):
    """x (B, Tin, Fin, Cin) channels-last, dY (B Tout Fout, Cout), dW base (n_store, K), db base (n_store,): float64"""
    Tin, Fin = conv_dims(c)
    M, N, K = conv_mnk(c)
    g = torch.Generator().manual_seed(77 + M * 7919 + c.Cin * 131 + N * 17 + K)
    return (_ints_nz((c.B, Tin, Fin, c.Cin), g), _ints_nz((M, N), g), torch.randint(-8, 9, (c.n_store, K), generator=g).double(),
            torch.randint(-8, 9, (c.n_store,), generator=g).double())


@functools.lru_cache(maxsize=2)
def conv_products(c):
    """float64 autograd of F.conv2d on the leading-padded input (generous trailing pad: windows that run past the input read zeros): the weight gradient in the
    kernel's layout (Cout, (kh, kw, c)), and the bias gradient"""
    x, dy, _, _ = conv_inputs(c)
    xp = F.pad(x.permute(0, 3, 1, 2), (c.pad_f, c.KW + 1, c.pad_t, c.KH + 1))
    w = torch.zeros(c.Cout, c.Cin, c.KH, c.KW, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xp, w, stride=c.stride)[:, :, :c.Tout, :c.Fout]
    y.backward(dy.view(c.B, c.Tout, c.Fout, c.Cout).permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).reshape(c.Cout, -1).contiguous(), dy.sum(0)


def conv_reference(c, calls=1):
    _, _, bw, bb = conv_inputs(c)
    prod, col = conv_products(c)
    return bw + calls * prod[:c.n_store], bb + calls * col[:c.n_store]


def conv_im2col(c):
    """the im2col operand (M, K) float64 restated by index arithmetic: row (b, to, fo), column (kh, kw, c) = x[b][to * st - pad_t + kh][fo * st - pad_f + kw][c]"""
    x, _, _, _ = conv_inputs(c)
    Tin, Fin = conv_dims(c)
    xp = F.pad(x, (0, 0, c.pad_f, c.KW + 1, c.pad_t, c.KH + 1))
    cols = []
    for kh in range(c.KH):
        for kw in range(c.KW):
            cols.append(xp[:, kh:kh + c.stride * c.Tout:c.stride, kw:kw + c.stride * c.Fout:c.stride, :])
    return torch.stack(cols, 3).reshape(c.B * c.Tout * c.Fout, -1)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the grouped launch (mi_gemm_tn_group_ow_bf16 through ctypes: TnBatch runs fewer than 64 tiles one by one, so small grids are reachable only this way)
Prob = namedtuple("Prob", "M N K n_store db views")
GroupCase = namedtuple("GroupCase", "id tile_k overwrite problems")
GROUP_M = (1, 63, 64, 65, 128, 129, 192, 193, 257)                   # 1 ... 5 stages against ring depths 3 (256 x 128) and 2 (256 x 256)


def group_plan(c):
    """(xw, ring depth, blocks per problem)"""
    xw = group_xw(c.tile_k, [(p.M, p.N, p.K) for p in c.problems])
    return xw, (2 if xw == 256 else 3), tuple(cdiv(p.N, 256) * cdiv(p.K, xw) for p in c.problems)


def _build_group():
    cases = []
    mi = [0]

    def probs(shapes):
        out = []
        for N, K in shapes:
            M = GROUP_M[mi[0] % len(GROUP_M)]
            i = mi[0]
            mi[0] += 1
            out.append(Prob(M, N, K, _ns(i, N), i % 3 != 1, i % 2 == 1))
        return tuple(out)

    # (block count, [(N, K)]) per tile_k: 1, 7, 8, 9 and 13 blocks from 1, 2 and 3 problems of mixed N, K (N = 8: a tile of 8 rows; N = 264: two n tiles)
    small = {128: ((1, [(8, 8)]), (7, [(264, 264), (8, 72)]), (8, [(264, 136), (136, 264), (8, 8)]), (9, [(264, 264), (72, 136), (128, 128)]),
                   (13, [(264, 520), (136, 136), (8, 8)])),
             256: ((1, [(8, 8)]), (7, [(264, 520), (8, 72)]), (8, [(264, 264), (136, 520), (8, 8)]), (9, [(264, 520), (72, 264), (128, 128)]),
                   (13, [(264, 520), (264, 520), (8, 8)]))}
    for tk in (128, 256):
        mi[0] = 0
        for gi, (blocks, shapes) in enumerate(small[tk]):
            c = GroupCase(f"tk{tk}-b{blocks}-p{len(shapes)}-" + ("ow" if gi % 2 == 0 else "add"), tk, gi % 2 == 0, probs(shapes))
            assert sum(group_plan(c)[2]) == blocks, (c.id, group_plan(c))
            cases.append(c)
        # the tile0 search at 47 and 48 problems; block counts that are no multiple of 8 (52 and 53)
        for n, ow in ((47, True), (48, False)):
            shapes = [((264, 72) if i % 10 == 3 else (8 * (1 + i % 9), 8 * (1 + i % 7))) for i in range(n)]
            c = GroupCase(f"tk{tk}-p{n}-" + ("ow" if ow else "add"), tk, ow, probs(shapes))
            assert sum(group_plan(c)[2]) % 8 != 0
            cases.append(c)
    # tile_k = 0: fewer than 200 256-tiles -> 256 x 128; 200 or more (48 problems of 2 x 3 tiles, M = 65: two stages) -> 256 x 256
    mi[0] = 3
    cases.append(GroupCase("tk0-few-add", 0, False, probs([(264, 264), (72, 520), (8, 8)])))
    cases.append(GroupCase("tk0-many-ow", 0, True, tuple(Prob(65, 264, 520, (264, 259, 1)[i % 3], i % 2 == 0, i % 4 == 1) for i in range(48))))
    assert group_plan(cases[-2])[0] == 128 and group_plan(cases[-1])[0] == 256
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


GROUP_CASES = _build_group()


def prob_layout(p) -> TnLayout:
    return TnLayout(8, p.N + 24, 16, p.K + 24, 4, p.K + 12) if p.views else TnLayout(0, p.N, 0, p.K, 0, p.K)


@functools.lru_cache(maxsize=128)
def prob_inputs(p, i):
    """problem i of a group: (dY, X, dW base, db base, dY[:, :n_store].T @ X, column sums) float64"""
    g = torch.Generator().manual_seed(5 + 1000003 * p.M + 1009 * p.N + p.K + 131071 * i)
    dy, x = _ints_nz((p.M, p.N), g), _ints_nz((p.M, p.K), g)
    return (dy, x, torch.randint(-8, 9, (p.n_store, p.K), generator=g).double(), torch.randint(-8, 9, (p.n_store,), generator=g).double(),
            dy[:, :p.n_store].t() @ x, dy.sum(0)[:p.n_store])


# single-defect calls of mi_gemm_tn_group_ow_bf16 that must return MI_ERR_ARG: name -> (n, {array: {index: value}}, tile_k).  The base call: 3 good problems.
GROUP_REFUSALS = {
    "n = 0": (0, {}, 128), "n = 49": (49, {}, 128), "N % 8": (3, {"N": {1: 132}}, 128), "ldy % 8": (3, {"ldy": {2: 140}}, 128), "ldx % 8": (3, {"ldx": {0: 132}}, 256),
    "n_store > N": (3, {"n_store": {1: 137}}, 128), "tile_k = 64": (3, {}, 64), "n_store = 0": (3, {"n_store": {0: 0}}, 0),
}


# ----------------------------------------------------------------------------------------------------------------------------------------
# bgemm.  la / lb: 0 = k-contiguous operand ([row][k]), 1 = row-contiguous ([k][row], the transposing LDS read)
# guard: "" (both operands qualify for the branch-free loads) | "a_off4" | "b_off4" (base 4 elements off a 16-B boundary) | "a_ragged" | "b_ragged" (contiguous,
#        extent % 8 != 0, no row padding);  pad: elements of readable NaN padding behind an extent that is already a multiple of 8 (a ragged extent is always padded
#        to the next multiple of 8 when the operand is to stay on the branch-free form);  zswap: z2 is the OUTER batch stride;  c_view: C inside wider rows
BgCase = namedtuple("BgCase", "id la lb Z1 Z2 M N K out_f32 alpha accumulate guard pad zswap c_view")
BG_MN = (1, 63, 64, 65, 127, 128, 129, 130)
BG_K = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 129)        # one tile; the two tiles in flight; a third; odd tile counts — at TK = 32 and at TK = 64
BG_KBIG = 4096
OperandLayout = namedtuple("OperandLayout", "off size shape strides z1 z2 s_row s_k")     # shape / strides: the as_strided (Z1, Z2, row, k) view of a flat buffer


def operand_layout(mode, Z1, Z2, R, K, kind, pad, zswap) -> OperandLayout:
    """kind: "fast" | "off4" | "ragged".  A flat NaN buffer; the operand is an as_strided view of it.  Between two batch entries lies one more (NaN) outer row, except
    in the contiguous ragged form."""
    inner, outer = (K, R) if mode == 0 else (R, K)
    if kind == "ragged":
        assert inner % 8, "a ragged extent is no multiple of 8"
        ld, gap = inner, 0
    else:
        ld, gap = rup(inner, 8) + pad, 1
    zin = (outer + gap) * ld
    za, zb = (Z2 * zin, zin) if not zswap else (zin, Z1 * zin)
    off = 4 if kind == "off4" else 0
    size = off + (Z1 - 1) * za + (Z2 - 1) * zb + outer * ld + 8
    s_row, s_k = (ld, 1) if mode == 0 else (1, ld)
    return OperandLayout(off, size, (Z1, Z2, R, K), (za, zb, s_row, s_k), za, zb, s_row, s_k)


def bg_layouts(c):
    ka = {"a_off4": "off4", "a_ragged": "ragged"}.get(c.guard, "fast")
    kb = {"b_off4": "off4", "b_ragged": "ragged"}.get(c.guard, "fast")
    return (operand_layout(c.la, c.Z1, c.Z2, c.M, c.K, ka, c.pad, c.zswap), operand_layout(c.lb, c.Z1, c.Z2, c.N, c.K, kb, c.pad, not c.zswap))


CLayout = namedtuple("CLayout", "off size ldc z1 z2")


def c_layout(Z1, Z2, M, N, view) -> CLayout:
    ldc, off = (N + 12, 4) if view else (N, 0)
    z2 = (M + 1) * ldc                                  # one guard row between batch entries
    return CLayout(off, off + Z1 * Z2 * z2 + 8 * ldc, ldc, Z2 * z2, z2)


def bg_form(c):
    """(tile, fast): the instantiation is bgemm_kernel<la, lb, tile, tile / 2, fast>"""
    A, B = bg_layouts(c)
    fast = bg_operand_fast(A.off, A.z1, A.z2, A.s_row, A.s_k, c.M, c.K) and bg_operand_fast(B.off, B.z1, B.z2, B.s_row, B.s_k, c.N, c.K)
    return bg_tile(c.M, c.N, c.Z1 * c.Z2), fast


def _bg(la, lb, Z1, Z2, M, N, K, out_f32, alpha, acc, guard, pad, zswap, c_view):
    cid = (f"a{la}b{lb}-{Z1}x{Z2}-{M}x{N}x{K}-" + ("f32" if out_f32 else "bf16") + ("-half" if alpha == 0.5 else "") + ("-acc" if acc else "") + (f"-{guard}" if guard else "")
           + (f"-pad{pad}" if pad else "") + ("-zswap" if zswap else "") + ("-cview" if c_view else ""))
    return BgCase(cid, la, lb, Z1, Z2, M, N, K, bool(out_f32), alpha, bool(acc), guard, pad, bool(zswap), bool(c_view))


# the 128 tile needs M, N > 64 and >= 256 blocks: Z1 Z2 = 64 at M = N = 129 / 130 (four blocks each), or Z = 256 at M, N in (64, 128]
BG_128_SHAPES = ((8, 8, 130, 130), (16, 16, 65, 128), (8, 8, 129, 130), (16, 16, 127, 65), (16, 16, 128, 127), (8, 8, 130, 129))


def _guard_for(la, lb, M, N, K, i):
    """a guard kind for running number i that is possible at this shape (a ragged extent must be no multiple of 8)"""
    inner_a, inner_b = (K if la == 0 else M), (K if lb == 0 else N)
    for j in range(4):
        g = ("a_off4", "b_ragged", "b_off4", "a_ragged")[(i + j) % 4]
        if g == "a_ragged" and inner_a % 8 == 0 or g == "b_ragged" and inner_b % 8 == 0:
            continue
        return g


def _build_bg():
    cases = []
    i = 0
    for la in (0, 1):
        for lb in (0, 1):
            for tile in (64, 128):
                for fast in (True, False):
                    for ki, K in enumerate(BG_K):
                        if tile == 64:
                            Z1, Z2, M, N = 2, 3, BG_MN[(ki + 2 * la + lb) % 8], BG_MN[(3 * ki + la + 2 * lb + 1) % 8]
                        else:
                            Z1, Z2, M, N = BG_128_SHAPES[(ki + la + 2 * lb) % 6]
                        guard = "" if fast else _guard_for(la, lb, M, N, K, i)
                        cases.append(_bg(la, lb, Z1, Z2, M, N, K, i % 2 == 0, (1.0, 0.5)[(i // 2) % 2], (i // 3) % 2 == 1, guard, 8 * ((i // 2) % 2) if fast else 0,
                                         i % 3 == 0, i % 2 == 1 or i % 5 == 0))
                        i += 1
    # K = 4096, the exactness bound, once per tile
    cases.append(_bg(0, 1, 2, 3, 65, 63, BG_KBIG, True, 0.5, True, "", 0, False, True))
    cases.append(_bg(1, 0, 8, 8, 130, 130, BG_KBIG, False, 1.0, False, "", 8, True, False))
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


BG_CASES = _build_bg()


@functools.lru_cache(maxsize=4)
def _bg_operands(Z1, Z2, M, N, K):
    g = torch.Generator().manual_seed(13 + 1000003 * M + 1009 * N + K + 7 * Z1 + Z2)
    a = torch.randint(-3, 4, (Z1, Z2, M, K), generator=g).double()
    b = torch.randint(-3, 4, (Z1, Z2, N, K), generator=g).double()
    base = torch.randint(-8, 9, (Z1, Z2, M, N), generator=g).double()
    return a, b, base, torch.einsum("abmk,abnk->abmn", a, b)


def bg_inputs(c):
    a, b, base, _ = _bg_operands(c.Z1, c.Z2, c.M, c.N, c.K)
    return a, b, base if c.accumulate else None


def bg_reference(c):
    """float64 (Z1, Z2, M, N): alpha * A B^T (+ C).  Exact: a multiple of 0.5 below 2**24."""
    _, _, base, prod = _bg_operands(c.Z1, c.Z2, c.M, c.N, c.K)
    return c.alpha * prod + base if c.accumulate else c.alpha * prod


def bg_expected(ref, out_f32):
    """what the launch must leave, bit for bit: the float64 value in fp32, or its round-to-nearest-even bf16 cast"""
    return ref.to(torch.float32 if out_f32 else torch.bfloat16)


# the d(positions) product on real band_geometry layouts: A = dBD (H, G cg, Tt, Ps), row-contiguous along the relative position, banded along K = (u, i)
BandCase = namedtuple("BandCase", "id Tt cg hd H G guard")


def band_geometry(T):
    """ops_train.band_geometry"""
    pad = (32 - T) % 32
    return pad, (pad + 2 * T - 1 + 31) // 32 * 32


def band_form(c):
    off, Kp = band_geometry(c.Tt)
    return bg_tile(Kp, c.hd, c.H * c.G), c.guard == ""


BAND_T, BAND_CG = (31, 32, 33, 64, 65, 97), (1, 2, 3)
# every (Tt, cg) on the branch-free 64 tile (the only form that skips k tiles); one more with qv 4 elements off a 16-B boundary (the guarded kernel walks all of K:
# the band argument must change nothing); the 128 tile at hd = 128, H x G = 64
BAND_CASES = (tuple(BandCase(f"T{Tt}-cg{cg}-hd64", Tt, cg, 64, 2, 3, "") for Tt in BAND_T for cg in BAND_CG)
              + (BandCase("T65-cg2-hd64-b_off4", 65, 2, 64, 2, 3, "b_off4"), BandCase("T250-cg1-hd128-tile128", 250, 1, 128, 4, 16, "")))


@functools.lru_cache(maxsize=2)
def band_inputs(c):
    """dbd (H, G cg, Tt, Ps) with row i non-zero only in columns [Tt - 1 - i + off, 2 Tt - 1 - i + off) — true zeros outside —, qv (G cg Tt, H hd); float64 integers"""
    off, Ps = band_geometry(c.Tt)
    g = torch.Generator().manual_seed(3 + 131 * c.Tt + c.cg)
    ds = torch.randint(-3, 4, (c.H, c.G * c.cg, c.Tt, c.Tt), generator=g).double()
    dbd = torch.zeros(c.H, c.G * c.cg, c.Tt, Ps, dtype=torch.float64)
    for i in range(c.Tt):
        dbd[:, :, i, c.Tt - 1 - i + off: 2 * c.Tt - 1 - i + off] = ds[:, :, i, :]
    qv = torch.randint(-3, 4, (c.G * c.cg * c.Tt, c.H * c.hd), generator=g).double()
    return dbd, qv


def band_reference(c):
    """float64 (G, Kp * H * hd): the einsum of tests/test_gpu_train_ops.py test_bgemm_band_skips_only_zero_tiles"""
    dbd, qv = band_inputs(c)
    off, Kp = band_geometry(c.Tt)
    return torch.einsum("hbip,bihc->bphc", dbd.view(c.H, c.G, c.cg * c.Tt, Kp), qv.view(c.G, c.cg * c.Tt, c.H, c.hd)).reshape(c.G, Kp * c.H * c.hd)


# m_valid: batch entry z2 has lens[z2] live rows of A.  Rows at or past it inside a live tile are true zeros, whole dead tiles NaN.
MvCase = namedtuple("MvCase", "id la Z1 lens M N K out_f32 accumulate")


def mv_form(c):
    return bg_tile(c.M, c.N, c.Z1 * len(c.lens))


def _build_mv():
    cases = []
    for tile, Z1, M, N in ((64, 2, 200, 64), (128, 16, 300, 72)):
        lens = (0, 1, tile - 1, tile, tile + 1, M)                  # nothing, one row, a tile edge and its neighbours, everything
        for la, out_f32, acc in ((1, True, False), (1, False, True), (0, True, True), (0, False, False)):
            c = MvCase(f"t{tile}-a{la}-" + ("f32" if out_f32 else "bf16") + ("-acc" if acc else ""), la, Z1, lens, M, N, 72, out_f32, acc)
            assert mv_form(c) == tile
            cases.append(c)
    return tuple(cases)


MV_CASES = _build_mv()


@functools.lru_cache(maxsize=2)
def mv_inputs(c):
    """A (Z1, Z2, M, K) with rows >= lens[z2] zeroed, B (Z1, Z2, N, K), C base (Z1, Z2, M, N): float64"""
    Z2 = len(c.lens)
    g = torch.Generator().manual_seed(9 + c.M + 17 * c.Z1)
    a = torch.randint(-3, 4, (c.Z1, Z2, c.M, c.K), generator=g).double()
    for z, n in enumerate(c.lens):
        a[:, z, n:] = 0
    b = torch.randint(-3, 4, (c.Z1, Z2, c.N, c.K), generator=g).double()
    return a, b, torch.randint(-8, 9, (c.Z1, Z2, c.M, c.N), generator=g).double()


def mv_reference(c):
    a, b, base = mv_inputs(c)
    prod = torch.einsum("abmk,abnk->abmn", a, b)
    return prod + base if c.accumulate else prod


def mv_dead_rows(c, z):
    """first row of the first dead tile of batch entry z (M if none)"""
    return min(c.M, rup(c.lens[z], mv_form(c)))
