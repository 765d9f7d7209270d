#!/usr/bin/env python3
"""A canonical text dump of what the conv launch builder plans: `python tools/conv_plan_dump.py [OUT.txt]` (host only, no GPU).

Every entry of tests/conv_cases.py CONV_CASES at its own call shape and at B in {1, 2, 8, 32, 64} x L in {1, 20, 45, 150, 299,
1500} (a gemv case: L = 1), each also as the plan of ONE row of 1, 20, 45, 150, 299 or all frames of that call (plan_frames; the
stride-1 and transposed MFMA cases), every BLOCK_CASES block at the same shapes, and the REFUSED list.  A line is the case and
either the return code of a refusal or the whole record smi_conv_plan / smi_voc_block_plan report; the last line counts them.
The diagnostics library is the tree's own, or the one SPARKMI_LIB names: two builds plan alike when their dumps are equal.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spark-tts_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BS = (1, 2, 8, 32, 64)
LS = (1, 20, 45, 150, 299, 1500)


def plan_line(tag, case):
    from sparkmi import _lib, bicodec as B
    info = _lib.ConvPlanInfo()
    rc = _lib.diag().smi_conv_plan(C.byref(case), C.byref(info))
    if rc:
        return f"{tag} rc={rc}"
    return (f"{tag} {B.form_name(info.form.key())} #{info.form_index} xw={info.xw} grid={tuple(info.grid)} lout={info.lout} "
            f"lds={info.lds_bytes} plan_blocks={info.plan_blocks}")


def block_lines(tag, kind, kw, Bn, L, dil):
    from sparkmi import _lib, bicodec as B
    d = _lib.diag()
    cs = _lib.VocBlockCfg(kind=kind, C=kw["C_"], Cout=kw.get("Cout", 0), K=kw.get("K", 0), S=kw.get("S", 1), dil=dil, I=kw.get("I", 0))
    out = (_lib.BlockLaunchInfo * 16)()
    n = C.c_int32()
    rc = d.smi_voc_block_plan(C.byref(cs), Bn, L, out, 16, C.byref(n))
    if rc:
        return [f"{tag} rc={rc}"]
    return [f"{tag} [{i}] {o.name.decode()} kind={o.kind} " + (f"{B.form_name(o.form.key())} #{o.form_index}" if o.kind == 0 else
                                                                f"res_nwv={o.res_nwv} cpt={o.cpt}") for i, o in enumerate(out[: n.value])]


def dump():
    import conv_cases as cc
    from sparkmi.bicodec import conv_case
    lines = []
    for name, c in cc.CONV_CASES.items():
        mk = lambda Bn, Ln, pf=0: conv_case(c["Cout"], c["Cin"], c["K"], c["dil"], c["S"], c["istr"], c["act"], c["bf"], Bn, Ln,
                                            plan_frames=pf, gemv=c["gemv"], c1=c["c1"])
        shapes = [(c["B"], c["L"])] + [(Bn, Ln) for Bn in BS for Ln in ((1,) if c["gemv"] else LS)]
        for Bn, Ln in shapes:
            lines.append(plan_line(f"conv {name} B={Bn} L={Ln}", mk(Bn, Ln)))
            if c["gemv"] or c["c1"] or c["istr"] > 1:
                continue
            for pf in sorted({f for f in LS if f < Ln} | {Ln}):
                lines.append(plan_line(f"conv {name} B={Bn} L={Ln} plan_frames={pf}", mk(Bn, Ln, pf)))
    for name, (kind, kw, Bn0, L0, _) in cc.BLOCK_CASES.items():
        for dil in ((1, 3, 9) if kind == cc.BLOCK_RESUNIT else (1,)):
            for Bn, Ln in [(Bn0, L0)] + [(Bn, Ln) for Bn in BS for Ln in LS]:
                lines += block_lines(f"block {name} dil={dil} B={Bn} L={Ln}", kind, kw, Bn, Ln, dil)
    for name, (kw, _) in cc.REFUSED.items():
        lines.append(plan_line(f"refused {name}", conv_case(**kw)))
    lines.append(f"cases {len(lines)}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = dump()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
