#!/usr/bin/env python3
"""Generates fp256_addasm.inc: fp_add / fp_sub for gfx950 as one inline-asm statement each.

Why asm: the carry of the fold has to reach a wave-uniform "does any lane carry on?" branch.  From C the compiler
materialises the carry (v_cndmask 0/1) and compares it again (v_cmp_ne) before s_cbranch -- two VALU instructions per
test, three tests per butterfly.  Here the carry-outs stay lane masks and scalar instructions hand the rare lanes to the
caller, who tests them with scalar instructions only.  `s_nop 1` = the two wait states gfx950 needs between a VALU write
of VCC (or of an SGPR pair) and the VALU that reads it as a carry.

The fold, three VALU instructions.  With CY the carry out of limb 7 (in VCC), r += CY * c, c = 351 * 2^32 - 1, is
    r0 - CY                       borrow B0 = CY & [r0 == 0]            v_subb  r0, sB, r0, 0, vcc
    m = CY ? -0x15f : 0                                                 v_cndmask m, 0, K, vcc
    r1 - m - B0 = r1 + 0x15f CY - B0                                    v_subb  r1, sB, r1, m, sB
(c's limb 0 is 2^32 - 1 and its limb 1 plus one is 0x15f).  The last borrow is set exactly where CY is and limb 1 does NOT
carry out, so the rare lanes are CY & ~sB: one s_andn2 on the scalar unit.  fp_sub mirrors it (r0 + BW, carry C0, then
r1 + m + C0; rare lanes BW & ~carry).  gfx950 takes no literal in a VOP3 encoding and one scalar operand per VALU
instruction, and the lane mask is that one: K = -0x15f comes in a VGPR (an operand of the statement).
check() below interprets the emitted lines on integers, one lane per case and the rare lanes included, and checks the wait states."""
import os

K = 0xFFFFFEA1  # -0x15f


def chain(add):
    """operands: %0..%7 r, %8 m, %9 any(s64, also the fold's borrow / carry pair), %10..%17 a, %18..%25 b, %26 K"""
    first, nxt = ("v_add_co_u32_e32", "v_addc_co_u32_e32") if add else ("v_sub_co_u32_e32", "v_subb_co_u32_e32")
    fold = "v_subb_co_u32_e64" if add else "v_addc_co_u32_e64"
    L = []
    L.append("%s %%0, vcc, %%10, %%18" % first)
    for i in range(1, 8):
        L.append("s_nop 1")
        L.append("%s %%%d, vcc, %%%d, %%%d, vcc" % (nxt, i, 10 + i, 18 + i))
    L.append("s_nop 1")
    L.append("%s %%0, %%9, %%0, 0, vcc" % fold)       # limb 0 -/+ the carry (borrow); VCC keeps it
    L.append("v_cndmask_b32_e32 %8, 0, %26, vcc")      # m = carry ? -0x15f : 0
    L.append("s_nop 0")
    L.append("%s %%1, %%9, %%1, %%8, %%9" % fold)
    L.append("s_andn2_b64 %9, vcc, %9")                # lanes whose fold leaves limb 1
    return L


def check(lines, add):
    """the wait states, and the emitted lines interpreted against exact integers on one lane per case"""
    ws, last = 0, {}
    for ln in lines:
        op, args = ln.split(None, 1)
        args = [x.strip() for x in args.split(",")]
        if op == "s_nop":
            ws += int(args[0]) + 1
            continue
        if op.startswith("v_"):
            carry_in = {"v_addc_co_u32_e32": "vcc", "v_subb_co_u32_e32": "vcc", "v_cndmask_b32_e32": "vcc"}.get(op)
            if op.endswith("_e64"):
                carry_in = args[4]
            if carry_in is not None:
                assert carry_in in last and ws - last[carry_in] - 1 >= 2, ln
            if op != "v_cndmask_b32_e32":
                last[args[1]] = ws
        ws += 1
    # the emitted lines, interpreted on one lane: registers by operand name, lane masks as 0 / 1
    W, M64, M256 = 1 << 32, (1 << 64) - 1, 1 << 256
    c = 351 * W - 1
    edge1 = [0, 1, 0x15E, 0x15F, 0x160, 0xFFFFFEA0, 0xFFFFFEA1, 0xFFFFFEA2, 0xFFFFFFFF]
    edge0 = [0, 1, 0xFFFFFFFE, 0xFFFFFFFF]

    def run(a, b):
        R = {"%%%d" % (10 + i): (a >> (32 * i)) % W for i in range(8)}
        R.update({"%%%d" % (18 + i): (b >> (32 * i)) % W for i in range(8)})
        R["%26"] = K
        val = lambda x: R[x] if x in R else int(x, 0)
        for ln in lines:
            op, args = ln.split(None, 1)
            args = [x.strip() for x in args.split(",")]
            if op == "s_nop":
                continue
            if op == "s_andn2_b64":
                R[args[0]] = val(args[1]) & ~val(args[2]) & 1
            elif op == "v_cndmask_b32_e32":
                R[args[0]] = val(args[2]) if R[args[3]] else val(args[1])
            else:
                base = op.split("_co_")[0]  # v_add, v_addc, v_sub, v_subb
                cin = val(args[4]) if base in ("v_addc", "v_subb") else 0
                t = val(args[2]) + val(args[3]) + cin if base.startswith("v_add") else val(args[2]) - val(args[3]) - cin
                R[args[0]], R[args[1]] = t % W, int(not 0 <= t < W)
        return sum(R["%%%d" % i] << (32 * i) for i in range(8)), R["%9"]

    for top in (0, 1):
        for l1 in edge1:
            for l0 in edge0:
                for upper in (0, (1 << 192) - 1, 0x0123456789ABCDEF << 100):
                    s = l0 | (l1 << 32) | (upper << 64)     # the eight limbs before the fold
                    if add:
                        if top and s > M256 - 2:
                            continue
                        a = (s + 1 + (0x9E3779B97F4A7C15 << 150)) % (M256 - s - 1) + s + 1 if top else s // 3
                        b = s + top * M256 - a
                        lo = (s & M64) + top * c
                    else:
                        if top and s == 0:
                            continue
                        a = s // 3 if top else s + (M256 - s) // 5
                        b = a - s + top * M256
                        lo = (s & M64) - top * c
                    assert 0 <= a < M256 and 0 <= b < M256, (add, top, s)
                    want = (s & ~M64) | (lo & M64)           # limbs 0..1 folded, the rest untouched
                    rare = int(not 0 <= lo <= M64)            # the fold leaves limb 1
                    assert run(a, b) == (want, rare), (add, top, hex(s), hex(a), hex(b))


def emit(lines):
    outs = ", ".join('"=&v"(r.v[%d])' % i for i in range(8)) + ', "=&v"(m), "=&s"(any)'
    ins = ", ".join('"v"(a.v[%d])' % i for i in range(8)) + ", " + ", ".join('"v"(b.v[%d])' % i for i in range(8)) + ', "v"(k)'
    return ['  asm("%s"' % "\\n\\t".join(lines), "      : %s" % outs, "      : %s" % ins, '      : "vcc");']


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    L = ["// GENERATED by gen_addasm.py -- do not edit.  fp_add / fp_sub common paths as single asm statements (gfx950).",
         "// r = a + b (resp. a - b) over 8 limbs, then the fold of the carry (borrow) as +c (-c) on limbs 0..1;",
         "// returns the lane mask of carries (borrows) that leave limb 1 -- the rare continuation is the caller's (fp256.cuh)."]
    for add in (True, False):
        lines = chain(add)
        check(lines, add)
        L += ["__device__ __forceinline__ uint64_t fp_%s_asm(const fp& a, const fp& b, fp& r) {" % ("add" if add else "sub"),
              "  uint32_t m;", "  uint64_t any;", "  const uint32_t k = 0x%08xu;  // -0x15f" % K]
        L += emit(lines)
        L += ["  return any;", "}"]
    # six-limb sum with the carry-out as a lane mask (fp_reduce_13: lo + D)
    L += ["// r[0..5] = x[0..5] + y[0..5]; returns the lane mask of carries out of limb 5",
          "__device__ __forceinline__ uint64_t fp_add6_asm(const uint32_t* x, const uint32_t* y, uint32_t* r) {",
          "  uint64_t any;"]
    T = ["v_add_co_u32_e32 %0, vcc, %7, %13"]
    for i in range(1, 6):
        T += ["s_nop 1", "v_addc_co_u32_e32 %%%d, vcc, %%%d, %%%d, vcc" % (i, 7 + i, 13 + i)]
    T += ["s_mov_b64 %6, vcc"]
    outs = ", ".join('"=&v"(r[%d])' % i for i in range(6)) + ', "=s"(any)'
    ins = ", ".join('"v"(x[%d])' % i for i in range(6)) + ", " + ", ".join('"v"(y[%d])' % i for i in range(6))
    L += ['  asm("%s"' % "\\n\\t".join(T), "      : %s" % outs, "      : %s" % ins, '      : "vcc");', "  return any;", "}"]
    with open(os.path.join(here, "fp256_addasm.inc"), "w") as fh:
        fh.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
