"""Static instruction budget per kernel from a gfx950 assembly listing: what a wave of the kernel has to issue.

    hipcc <FLAGS of csrc/build.py> --cuda-device-only -S huggingface_asr_amd/csrc/conv.hip -o conv.s
    python tools/isa_budget.py conv.s dwconv31_kernel [more name fragments ...]

Per kernel whose (mangled) name contains a fragment: instruction count, FMAs (v_fma* / v_fmac*), transcendentals (v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos),
other VALU, SALU (waits, barriers and nops counted apart), branches, every LDS opcode and every global / buffer opcode with its count, VGPRs, SGPRs, scratch bytes, and —
for the depthwise-conv kernels, whose tap chains are everything between the barrier after the fill and the next one — the branches between the first and the last FMA of
the section that holds the most FMAs (`tap-section branches`).  Counts are static: a kernel without loops executes each instruction at most once per wave.
"""
import collections
import re
import sys

TRANS = re.compile(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_")
SYNC = ("s_waitcnt", "s_barrier", "s_nop", "s_endpgm", "s_sleep", "s_setprio", "s_code_end")


def kernels(path):
    """-> {name: [instruction mnemonics in program order]}, {name: {metadata key: value}}"""
    body, meta, cur = collections.OrderedDict(), collections.defaultdict(dict), None
    mname = None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):", s)
        if m:                                                  # a function label opens a body; .Lfunc_end closes it (a kernel may hold several s_endpgm)
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if s.startswith(".name:"):
            mname = s.split(":", 1)[1].strip()
        for key in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".agpr_count"):
            if s.startswith(key + ":") and mname:
                meta[mname][key] = int(s.split(":", 1)[1])
        if cur is None or not s or s.startswith((".", ";", "/")):
            continue
        op = s.split()[0]
        if re.match(r"^(v_|s_|ds_|global_|buffer_|flat_|scratch_)", op):
            body[cur].append(op)
    return body, meta


def budget(ops):
    c = collections.Counter()
    mem = collections.Counter()
    for op in ops:
        if op.startswith(("v_fma", "v_fmac")):
            c["fma"] += 1
        elif TRANS.match(op):
            c["transcendental"] += 1
        elif op.startswith("v_"):
            c["other VALU"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["branches"] += 1
        elif op.startswith(SYNC):
            c["waits/barriers/nops"] += 1
        elif op.startswith("s_"):
            c["SALU+SMEM"] += 1
        else:
            mem[op] += 1
    # the section (between barriers) with the most FMAs, and the branches between its first and last FMA
    sections, cur = [], []
    for op in ops:
        if op == "s_barrier":
            sections.append(cur); cur = []
        else:
            cur.append(op)
    sections.append(cur)
    isf = lambda o: o.startswith(("v_fma", "v_fmac"))
    best = max(sections, key=lambda sec: sum(isf(o) for o in sec))
    idx = [i for i, o in enumerate(best) if isf(o)]
    tap_br = sum(o.startswith(("s_cbranch", "s_branch")) for o in best[idx[0]:idx[-1] + 1]) if idx else 0
    tap = collections.Counter()
    if idx:
        for o in best[idx[0]:idx[-1] + 1]:
            tap["fma" if isf(o) else "transcendental" if TRANS.match(o) else "VALU" if o.startswith("v_") else "LDS" if o.startswith("ds_") else "scalar/other"] += 1
    return c, mem, tap_br, tap


def main():
    path, frags = sys.argv[1], sys.argv[2:] or [""]
    body, meta = kernels(path)
    for name, ops in body.items():
        if not any(f in name for f in frags) or not ops:
            continue
        c, mem, tap_br, tap = budget(ops)
        md = meta.get(name, {})
        print(name)
        print(f"  instructions {len(ops)}: fma {c['fma']}, other VALU {c['other VALU']}, transcendental {c['transcendental']}, SALU+SMEM {c['SALU+SMEM']}, "
              f"branches {c['branches']}, waits/barriers/nops {c['waits/barriers/nops']}, memory {sum(mem.values())}")
        print("  memory ops: " + ", ".join(f"{k} {v}" for k, v in sorted(mem.items())))
        print(f"  tap section (first to last FMA between two barriers): " + ", ".join(f"{k} {v}" for k, v in sorted(tap.items())) + f"; branches {tap_br}")
        print(f"  VGPRs {md.get('.vgpr_count')}, AGPRs {md.get('.agpr_count', 0)}, SGPRs {md.get('.sgpr_count')}, scratch {md.get('.private_segment_fixed_size')} B, "
              f"static LDS {md.get('.group_segment_fixed_size')} B")


if __name__ == "__main__":
    main()
