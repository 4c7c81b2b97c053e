#!/usr/bin/env python3
"""Static metrics of a conv_fwd9_kernel Winograd instantiation from the device assembly that `hipcc -save-temps` leaves
(conv_fwd9_k-hip-amdgcn-amd-amdhsa-gfx950.s).  A development aid, not a test.

  python tools/f9_asm_metrics.py FILE.s [kernel-name-substring]

Prints, for the (first matching) kernel:
  * the instructions between every s_barrier and the next v_mfma, how many of them are buffer_load (LDS-DMA issues) or VALU integer
    (address arithmetic), and the histogram of those counts (the step heads of the chunk loop: the matrix pipe is empty there);
  * the static instruction count behind the last v_mfma (the tile epilogue and the loop tails);
  * v_accvgpr_read / _write between the first and the last v_mfma: not zero means the register allocator parked fragments in AGPRs
    and copies them back inside the chunk loop (seen on small edits of the step macros: the plain build then runs at half speed);
  * MFMA-to-MFMA gaps under a crude issue model -- 4 cycles per VALU op, 16 per v_exp / v_rcp, 8 per v_pk_*, 64 per MFMA: the gaps
    longer than one MFMA, their total excess, and the gaps that hold more than one v_exp or v_rcp."""
import collections
import re
import sys


def instructions(path, want):
    ins, on = [], False
    for ln in open(path):
        s = ln.split(";")[0].strip()
        if not on:
            if s.endswith(":") and s.startswith("_Z") and want in s and "conv_fwd9_kernel" in s:
                on = True
            continue
        if s.startswith(".Lfunc_end"):
            break
        if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
            continue
        ins.append(s.split()[0])
    return ins


def main():
    path = sys.argv[1]
    ins = instructions(path, sys.argv[2] if len(sys.argv) > 2 else "")
    if not ins:
        sys.exit("no conv_fwd9_kernel instantiation found")
    mf = [i for i, op in enumerate(ins) if op.startswith("v_mfma")]
    print(f"{len(ins)} instructions, {len(mf)} v_mfma, {sum(op == 's_barrier' for op in ins)} s_barrier")
    # ---- step heads ----
    heads = []
    for i, op in enumerate(ins):
        if op != "s_barrier":
            continue
        j = i + 1
        while j < len(ins) and not ins[j].startswith("v_mfma") and ins[j] != "s_barrier":
            j += 1
        if j < len(ins) and ins[j].startswith("v_mfma"):
            seg = ins[i + 1:j]
            heads.append((len(seg), sum(o.startswith("buffer_load") for o in seg),
                          sum(bool(re.match(r"v_(add|sub|or|and|lshl|mul_lo|mad_u|cndmask|cmp)", o)) for o in seg),
                          sum(o.startswith("ds_read") for o in seg)))
    hist = collections.Counter(h[0] for h in heads)
    print(f"barrier -> next MFMA: {len(heads)} heads, instructions {dict(sorted(hist.items()))}")
    print(f"  heads with a buffer_load: {sum(h[1] > 0 for h in heads)}, with integer VALU: {sum(h[2] > 0 for h in heads)}, "
          f"with ds_read: {sum(h[3] > 0 for h in heads)}; instructions in all heads: {sum(h[0] for h in heads)}")
    # ---- epilogue ----
    print(f"instructions behind the last v_mfma: {len(ins) - 1 - mf[-1]}")
    print(f"v_accvgpr copies inside the MFMA range: {sum(op.startswith('v_accvgpr') for op in ins[mf[0]:mf[-1]])}")
    # ---- MFMA gaps ----
    def cost(op):
        if op.startswith("v_mfma"):
            return 0
        if op.startswith(("v_exp", "v_rcp", "v_log", "v_sqrt", "v_rsq")):
            return 16
        if op.startswith("v_pk_"):
            return 8
        if op.startswith("v_"):
            return 4
        return 0
    long_gaps, excess, crowded = 0, 0, 0
    for a, b in zip(mf, mf[1:]):
        seg = ins[a + 1:b]
        if "s_barrier" in seg or any(o.startswith(("s_cbranch", "s_branch")) for o in seg):
            continue
        c = sum(cost(o) for o in seg)
        if c > 64:
            long_gaps += 1
            excess += c - 64
        if sum(o.startswith("v_exp") for o in seg) > 1 or sum(o.startswith("v_rcp") for o in seg) > 1:
            crowded += 1
    print(f"MFMA gaps longer than 64 cycles of VALU issue: {long_gaps}, total excess {excess} cycles; gaps with more than one "
          f"v_exp or v_rcp: {crowded}")


if __name__ == "__main__":
    main()
