"""Which conv kernel form runs which case -- checked on the host.  The launch builder's choices (make_conv + the dispatch
of run_launch, csrc/smi_net.h) are read through the diagnostics library's host-only plan entries; the case table of
tests/conv_cases.py must reach every instantiated form, and its float64 reference with the derived bound must be able to
tell a subtly wrong kernel from a right one.  tests/test_conv_forms_gpu.py runs the same cases on the kernels."""
import numpy as np
import pytest
import torch

import conv_cases as cc
from sparkmi import bicodec as B


@pytest.fixture(scope="module")
def forms():
    return [B.form_name(f) for f in B.conv_forms()]


@pytest.fixture(scope="module")
def plans():
    return {n: B.plan_conv(cc.make_case(n)) for n in cc.CONV_CASES}


def test_form_table_is_a_set(forms):
    assert len(forms) == len(set(forms)) == 39


def test_every_case_plans_the_form_it_names(plans):
    for n, c in cc.CONV_CASES.items():
        assert B.form_name(plans[n].form.key()) == c["form"], n
        assert plans[n].lds_bytes <= 64 * 1024 and plans[n].xw <= 64 * max(1, plans[n].form.nc), n


def test_single_conv_cases_reach_every_reachable_form(forms, plans):
    """a form added to the table without a case fails here; so does a form listed as unreachable that a case reaches"""
    reached = {B.form_name(p.form.key()) for p in plans.values()}
    assert set(cc.UNREACHABLE) <= set(forms)
    assert reached == set(forms) - set(cc.UNREACHABLE), (sorted(set(forms) - set(cc.UNREACHABLE) - reached), sorted(reached & set(cc.UNREACHABLE)))
    for reason in cc.UNREACHABLE.values():
        assert "`" in reason     # quotes the builder condition


def test_unreachable_forms_are_excluded_by_the_builder():
    """128-channel chunks on the exact pipe without the channel split: a sweep over the shapes that decide (ks, chg) finds none"""
    for Cout in (32, 96, 250, 1024):
        for Cin in (128, 136, 1024):
            for (Bn, L) in [(1, 20), (3, 45), (16, 2021), (512, 27), (2048, 27), (64, 4000)]:
                f = B.plan_conv(B.conv_case(Cout, Cin, 1, B=Bn, L=L)).form
                assert not (f.kernel == 0 and f.chg == 4 and not f.ks)


def test_builder_refuses_what_no_kernel_runs():
    """the REFUSED list: a staged row wider than the form's passes, k_conv_c1 / k_gemv1 asked for a layer they cannot run -- each
    refused for that reason, before any launch; a residual keeps a k_convbT-shaped layer on k_convb.  The same layers without
    the offending property plan."""
    why = {"chg4_wide": "stages 127 columns", "strided_wide": "stages 323 columns", "c1_cout2": "k_conv_c1", "c1_residual": "k_conv_c1",
           "gemv_bf": "vector projection"}
    assert set(why) == {n for n, (_, want) in cc.REFUSED.items() if want is None}
    for n, (kw, want) in cc.REFUSED.items():
        if want is None:
            with pytest.raises(Exception, match=why[n]):
                B.plan_conv(B.conv_case(**kw))
        else:
            assert B.form_name(B.plan_conv(B.conv_case(**kw)).form.key()) == want, n
    ok = {"chg4_wide": dict(L=499), "strided_wide": dict(L=138), "c1_cout2": dict(Cout=1), "c1_residual": dict(has_R=False),
          "gemv_bf": dict(bf=False), "bT4_residual": dict(has_R=False)}
    for n, fix in ok.items():
        p = B.plan_conv(B.conv_case(**{**cc.REFUSED[n][0], **fix}))
        assert p.form_index >= 0 and p.xw <= 64 * max(1, p.form.nc), n
    assert B.form_name(B.plan_conv(B.conv_case(**{**cc.REFUSED["bT4_residual"][0], "has_R": False})).form.key()) == "k_convbT<4>"


def test_case_mix_per_form(forms, plans):
    """every form has a ragged case with L no multiple of 32, Cin no multiple of its chunk and a row ending inside a tile"""
    good = set()
    for n, c in cc.CONV_CASES.items():
        f = c["form"]
        lens = cc.case_lens(n)
        olens = [cc.out_len(c, v) for v in lens]
        if c["gemv"]:
            good.add(f)      # one vector per utterance: no time axis
            continue
        ragged = len(set(lens)) > 1 and any(o % 32 for o in (lens if c["S"] > 1 else olens))
        if c["L"] % 32 and c["Cin"] % cc.form_chunk(f) and ragged:
            good.add(f)
    assert good == set(forms) - set(cc.UNREACHABLE), sorted(set(forms) - set(cc.UNREACHABLE) - good)
    assert all(cc.reduction_length(c) <= 2048 for c in cc.CONV_CASES.values())


def test_block_cases_reach_the_fused_and_wide_forms():
    """both k_resunit wave counts and the two-launch unit at the same C in channel-split mode; k_convbT with 4 and 5 phases; the
    64- and 128-channel-chunk k_convb forms; every k_dwln width a ConvNeXt block reaches (its C <= 512 limit leaves 16 channels per
    thread as the widest: the 32-per-thread form serves the encoder's 1024-channel LayerNorms only)"""
    res, cpts, first = set(), set(), {}
    for n, (kind, kw, Bn, L, want) in cc.BLOCK_CASES.items():
        for dil in ((1, 3, 9) if kind == cc.BLOCK_RESUNIT else (1,)):
            pl = B.plan_block(kind, Bn, L, dil=dil, **kw)
            if "res_nwv" in want:
                assert [p["kind"] for p in pl] == [5] and pl[0]["res_nwv"] == want["res_nwv"], (n, dil, pl)
                res.add(want["res_nwv"])
            elif kind == cc.BLOCK_RESUNIT:
                assert [p["kind"] for p in pl] == [0, 0] and all(p["form"][2] == 1 for p in pl), (n, dil, pl)   # two launches, ks
            elif kind == cc.BLOCK_DECBLOCK:
                assert B.form_name(pl[0]["form"]) == want["forms"][0], (n, pl[0])
                first[n] = B.form_name(pl[0]["form"])
            else:
                assert pl[0]["kind"] == 1 and pl[0]["cpt"] == want["cpt"], (n, pl[0])
                cpts.add(pl[0]["cpt"])
    assert res == {3, 6} and cpts == {4, 12, 16}
    assert set(first.values()) == {"k_convbT<4>", "k_convbT<5>", "k_convb<qb1,co,chg4,nc1>", "k_convb<qb2,co,chg2,nc2>"}
    with pytest.raises(Exception):
        B.plan_block(cc.BLOCK_CONVNEXT, 2, 45, C_=1024, I=72)


@pytest.mark.parametrize("name", list(cc.CONV_CASES))
def test_reference_and_bound_discriminate(name):
    """the acceptance test passes the exact float64 result rounded to fp32 and rejects one dropped tap, one dropped input channel
    of the last chunk, and a last tile shifted by one column"""
    c = cc.CONV_CASES[name]
    ref, mag, lens, olens = cc.reference(name)
    ok, worst = cc.accept(c, ref.to(torch.float32).numpy(), ref, mag, olens)
    assert ok and worst < 1.0, worst
    for what, bad in cc.corruptions(name).items():
        ok, worst = cc.accept(c, bad.to(torch.float32).numpy(), ref, mag, olens)
        assert not ok, f"{what} passes the bound (worst ratio {worst})"
