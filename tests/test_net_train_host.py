"""CPU side of the probe of the actor's and the critic's training kernels (tests/net_train_cases.py): the host-only plan
(pnpx_net_train_probe_plan) against a plain restatement of pieces, chunks per piece and refusals; the case tables against the branches
they were chosen for; the emulations against the float64 references; the derived bars against profiles/net_train_probe.md; and the
mutants each bar must catch.  No GPU."""
import os
import re

import pytest
import torch

from tests import net_train_cases as NT

ROOT = NT.ROOT


def test_symbols_are_declared_and_bound():
    from tfpnp_amd import _lib
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    for name in ("pnpx_net_train_probe", "pnpx_net_train_probe_plan"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name), name
    body = re.search(r"typedef struct pnpx_net_train_probe_desc \{(.*?)\} pnpx_net_train_probe_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?(unsigned|void|float|int|double)\s*", "", decl.strip())
        names += [n.strip(" *\n") for n in decl.split(",") if n.strip()]
    assert names == [f[0] for f in _lib.NetTrainProbeDesc._fields_], names
    ops = re.search(r"enum pnpx_net_train_op \{(.*?)\};", header, flags=re.S).group(1)
    assert [n for n, _ in re.findall(r"PNPX_NT_(\w+) = (\d+)", ops)] == list(NT.OP_NAMES)


def test_walks_launch_through_the_shared_launchers():
    """Each of the 16 kernels is launched from one place, its launcher; the walks and the probe call the launchers."""
    csrc = os.path.join(ROOT, "tfpnp_amd", "csrc")
    kernels = {"policy_bn.hip": ("bn_partial_kernel", "bn_finish_kernel", "bn_apply_kernel"),
               "policy_grad.hip": ("pol_head_grad_kernel", "pol_head_param_grad_kernel", "pol_grad_seed_kernel", "bn_bwd_partial_kernel",
                                   "bn_bwd_finish_kernel", "bn_bwd_apply_kernel", "pol_wgrad_finish_kernel"),
               "critic_grad.hip": ("critic_wgrad_kernel", "critic_wn_grad_kernel", "critic_clip_mask_kernel", "critic_alpha_dot_kernel",
                                   "critic_fc_grad_kernel", "critic_alpha_finish_kernel")}
    assert sum(len(v) for v in kernels.values()) == 16
    for name, ks in kernels.items():
        src = open(os.path.join(csrc, name)).read()
        for k in ks:
            assert src.count("hipLaunchKernelGGL(%s," % k) == 1, (name, k)
    walk = open(os.path.join(csrc, "policy_bn.hip")).read()
    assert walk.count("launch_bn_stats(J, s)") == 1 and walk.count("launch_bn_apply(J, s)") == 1
    probe = open(os.path.join(csrc, "net_train_probe.hip")).read()
    for fn in ("launch_bn_stats", "launch_bn_apply", "launch_bn_bwd", "launch_critic_wgrad", "launch_pol_wgrad_finish", "launch_critic_wn_grad",
               "launch_critic_clip_mask", "launch_critic_alpha_dot", "launch_critic_fc_grad", "launch_critic_alpha_finish", "launch_pol_head_grad",
               "launch_pol_grad_seed"):
        assert fn + "(" in probe, fn
    assert "hipLaunchKernelGGL" not in probe


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan

def _wg_kw(c):
    return dict(B=c.B, h=c.h, w=c.w, cout=c.cout, K=c.K, cin=c.cin, Cp=c.Cp, kind=c.kind, Gg=c.Gg, Xg=c.Xg, inv_w=NT.WG_INV_W,
                inv_b=NT.WG_INV_B if c.wn else 0.0)


def test_plan_of_every_op_and_its_refusals():
    shapes = (dict(B=2, G=1, h=4, w=6), dict(B=2, h=4, w=6), dict(B=3), dict(B=0, G=1, h=4, w=6), dict(B=2, G=1, h=0, w=6), dict(B=2, G=0, h=3, w=3),
              dict(B=1, G=2, h=33, w=63), dict(B=3, G=1, h=40, w=37, momentum=0.5, update=1), dict(B=1, G=1, h=1, w=1, update=1),
              dict(B=2, G=1, h=4, w=6, momentum=1.5), dict(B=2, G=1, h=4, w=6, boost=8.0), dict(B=2, G=1, h=4, w=6, boost=3.0),
              dict(B=2, h=4, w=6, boost=2.0), dict(B=2, h=4, w=6, boost=-2.0), dict(B=2, G=1, h=4, w=6, thr=5.0), dict(B=2, h=1, w=2, thr=5.0),
              dict(B=2, G=4, h=4, w=6, resG=2, mG=3), dict(B=2, G=4, h=4, w=6, resG=3, mG=2), dict(B=2, G=4, h=4, w=6, resG=0, mG=2),
              dict(B=2, h=1, w=2, n_det=10), dict(B=2, h=1, w=2, n_det=15, spi=1), dict(B=2, h=1, w=2, n_det=65), dict(B=2, h=1, w=2, n_det=10, spi=2),
              dict(B=5, inv_w=0.5), dict(B=5, h=2, w=2, inv_w=0.5), dict(B=4097, G=1, h=64, w=64), dict(B=2, G=1, h=4, w=6, inv_b=1.0))
    shapes += tuple(_wg_kw(c) for c in NT.WGRAD_CASES[:3] + NT.WGRAD_CASES[8:10] + NT.WGRAD_CASES[-2:])
    base = _wg_kw(NT.WGRAD_CASES[0])
    shapes += tuple(dict(base, **bad) for bad in (dict(cout=48), dict(K=16), dict(kind=3), dict(cin=33), dict(Cp=8), dict(Gg=3), dict(Xg=3), dict(inv_w=0.0),
                                                  dict(kind=1, Cp=8, cin=9), dict(kind=1, Cp=8, cin=5), dict(kind=1, Cp=16), dict(G=1)))
    ran = set()
    for op in range(-1, 12):
        for kw in shapes:
            got = NT.plan(op, **kw)
            assert got == NT.plan_py(op, **kw), (op, kw, got)
            if got:
                ran.add(op)
    assert ran == set(range(11))             # every op runs on some shape of the list, and the unknown ones on none


def test_plan_pieces_of_the_case_tables():
    """The branches the shapes were chosen for: the weight gradient's pieces and chunks, the BatchNorm pieces, the head rows."""
    seen = {}
    for c in NT.WGRAD_CASES:
        v = NT.plan(NT.WGRAD_WN if c.wn else NT.WGRAD_PLAIN, **_wg_kw(c))
        assert v and (v & 255, v >> 8) == NT.wgrad_pieces(c.cout, c.K, c.B, c.h, c.w), c.name
        seen[(c.cout, c.K, c.B, c.h, c.w)] = (v & 255, v >> 8)
    assert tuple(seen[s][0] for s in NT.WG_SHAPES) == NT.WG_PIECES
    nch = lambda s: -(-s[2] * s[3] * s[4] // 32)
    assert (nch(NT.WG_SHAPES[1]), seen[NT.WG_SHAPES[1]]) == (5, (2, 3)) and 1 * 12 * 13 - 4 * 32 == 28       # chunks 3 + 2, the last with 28 live pixels
    assert (nch(NT.WG_SHAPES[2]), seen[NT.WG_SHAPES[2]]) == (7, (3, 3))                                      # chunks 3 + 3 + 1
    assert (6 * 10) % 32 != 0 and seen[NT.WG_SHAPES[3]] == (3, 2)                                            # chunks straddle rows and images
    assert seen[NT.WG_SHAPES[7]][0] == 1 and (512 // 32) ** 2 == 256
    for k in (0, 1, 2):       # every kind on the first four shapes; nt = 9, 4, 1
        assert {(c.cout, c.K, c.B, c.h, c.w) for c in NT.WGRAD_CASES if c.kind == k and not c.wn} >= set(NT.WG_SHAPES[:4])
    assert [len(NT.window_taps(k)) for k in (0, 1, 2)] == [9, 4, 1]
    assert any(c.kind == 1 and c.cin == 9 and c.Cp == 16 for c in NT.WGRAD_CASES)                # the stem: 9 inputs in 16 padded channels
    assert all(c.Xg == 4 * c.K // 8 for c in NT.WGRAD_CASES if c.kind == 2)
    assert sum(c.Gg > c.cout // 8 for c in NT.WGRAD_CASES) == 1
    want = {(2, 8, 2, 3): 1, (2, 1, 32, 32): 1, (1, 2, 33, 63): 2, (3, 1, 40, 37): 3, (2, 64, 2, 2): 1, (2, 3, 4, 6): 1}
    assert 1 * 33 * 63 - 2048 == 31 and 2 * 32 * 32 == 2048
    for cases, op in ((NT.STATS_CASES, NT.BN_STATS), (NT.BWD_CASES, NT.BN_BWD)):
        got = {}
        for c in cases:
            kw = dict(B=c.B, G=c.G, h=c.h, w=c.w)
            if op == NT.BN_STATS:
                kw.update(momentum=c.momentum, update=c.update)
            else:
                kw.update(boost=c.boost)
            got[(c.B, c.G, c.h, c.w)] = NT.plan(op, **kw)
            assert got[(c.B, c.G, c.h, c.w)] == NT.bn_pieces(c.B, c.h, c.w), c.name
        assert all(got[s] == n for s, n in want.items())
    for c in NT.APPLY_CASES:
        assert NT.plan(NT.BN_APPLY, B=c.B, G=c.G, h=c.h, w=c.w) == -(-c.B * c.G * c.h * c.w // 256)
    assert {(c.two, c.res, c.out, c.s2d) for c in NT.APPLY_CASES} >= {(t, r, o, s) for _, t, r in NT._FORMS for o, s in ((1, 0), (0, 1), (1, 1))}
    assert {(c.two, c.dy_out) for c in NT.BWD_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    for c in NT.HEAD_CASES:
        assert NT.plan(NT.HEAD_GRAD, B=c.B, h=c.h, w=c.w, n_det=c.n_det, spi=c.spi) == 2 + (64 + c.n_det if c.spi else c.n_det)
    assert {(c.n_det, c.spi) for c in NT.HEAD_CASES} == {(10, 0), (15, 0), (10, 1), (15, 1)} and {c.B for c in NT.HEAD_CASES} == {2, 5}


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

def test_inputs_are_representable_and_free_of_kinks():
    for c in NT.APPLY_CASES:
        d = NT.apply_inputs(c.name)
        for k in ("z0", "z1", "res"):
            if k in d:
                assert torch.equal(d[k], NT.q(d[k])), (c.name, k)
        pre = NT.apply_reference(c, d)["pre"]
        assert bool((pre[:, 2] == 0).all())                                   # the deliberate exact zeros
        rest = torch.cat([pre[:, :2], pre[:, 3:]], 1)
        assert float(rest.abs().min()) >= 1e-3 and bool((rest < 0).any()) and bool((rest > 0).any()), c.name
    for c in NT.BWD_CASES:
        d = NT.bwd_inputs(c.name)
        a = d["act"].view(-1)
        assert a[0] == 0 and a[1] == 0 and not torch.signbit(a[0]) and torch.signbit(a[1]) and a[2] < 0
        for k in ("g", "act", "z0", "z1"):
            if k in d:
                assert torch.equal(d[k], NT.q(d[k])), (c.name, k)
        big = max(float(v[0].abs().max()) for k, v in NT.bwd_reference(c, d).items() if k.startswith("dz"))
        assert big > 2 * NT.RANGE_LIMIT if c.trip else big < 0.5 * NT.RANGE_LIMIT, (c.name, big)
    for c in NT.STATS_CASES:
        z = NT.stats_inputs(c.name)["z0"].double()
        assert float(z[:, 1].var()) == 0 and abs(float(z[:, 0].mean())) > 50 * float(z[:, 0].std())
    for c in NT.WGRAD_CASES:
        d = NT.wgrad_inputs(c.name)
        gv = d["gv"].tolist()
        assert len(set(gv)) == c.B and (c.B < 2 or min(gv) < 0) and (c.B < 3 or 0.0 in gv), c.name
        if c.kind == 1 and c.cin < c.Cp:
            X = d["X"].view(c.B, 4, c.Cp, c.h, c.w)
            assert bool((X[:, :, c.cin:] == 0).all()) and bool((X[:, :, :c.cin] != 0).all())
    for c in NT.HEAD_CASES:
        d = NT.head_inputs(c.name)
        if c.spi:
            pre = d["feat"].double().mean((2, 3)) @ d["d_w"].double().t() + d["d_b"].double()
            assert float(pre.abs().min()) >= 0.05 and bool((pre[:, :4] < -1).all()) and bool((pre > 0).any())
    for c in NT.CLIP_CASES + NT.FC_CASES:
        st = NT.clip_inputs(c.name)["act"].double() * NT.ASCALE
        assert bool((st == NT.THR).any()) and bool((st > NT.THR).any()) and bool((st < NT.THR).any())
    assert any(s < 0 for s in NT.fin_inputs("fin_B5")["alpha_src"])
    m = [float(NT.seed_inputs(c.name)["gf"].abs().max()) for c in NT.SEED_CASES]
    assert m[0] == 0.25 and 0.99999 < m[1] < 1 and m[2] == 0 and NT.SEED_CASES[3].boost != 1 and m[4] == 0.75


# ---------------------------------------------------------------------------------------------------------------------------------
# references, emulations, bars

def test_recorded_bars_are_eight_times_the_emulation_maxima():
    rec, emu = NT.recorded_bars(), NT.emulation_maxima()
    for k in NT.DERIVED_KEYS:
        mx, b = rec[k]
        assert emu[k][0] == pytest.approx(mx, rel=1e-4), (k, emu[k])          # the file holds 5 significant digits
        assert b == pytest.approx(NT.BAR_FACTOR * emu[k][0], rel=1e-4), k
        assert NT.bar(k) == b
        assert 2.0 ** -27 < mx < 2.0 ** -19, (k, mx)      # fp32 noise, not an error: between an eighth of and 32 unit roundoffs
    for k, (n, _) in NT.FIXED_BARS.items():
        assert NT.bar(k) == n * 2.0 ** -24 and 1 <= n <= 4


def test_weight_gradient_reference_is_the_correlation_the_kernel_documents():
    """autograd through conv2d (stride 2 over the full-resolution input for kinds 1 and 2) = sum_b gv[b] G[b] X[b, tap] gathered through
    eff_pos_of_src: the restated phase / tap map and the space-to-depth layout agree with the convolution."""
    for c in NT.WGRAD_CASES:
        if c.wn or c.cout > 64:
            continue
        d = NT.wgrad_inputs(c.name)
        ref, den = NT.wgrad_reference(c, d)["dw"]
        Gs, Xt = NT.wgrad_operands(c, d)
        Gv = (Gs * d["gv"].double().view(c.B, 1, 1, 1)).permute(1, 0, 2, 3).reshape(c.cout, -1)
        E = torch.einsum("cp,tkp->ctk", Gv, Xt.permute(0, 2, 1, 3, 4).reshape(Xt.shape[0], c.K, -1))
        direct = NT._gather(c, E) * NT.WG_INV_W
        assert NT.measure(direct, ref, den) < 1e-13, c.name
        assert bool((den > 0).all())


def _stats_one_pass(c, d):
    """bn_partial / bn_finish restated: one pass in double, var = q / n - mean^2 clamped at 0, the stores to fp32."""
    z = d["z0"].double()
    C, n = z.shape[1], z.numel() // z.shape[1]
    zf = z.permute(1, 0, 2, 3).reshape(C, n)
    P = d["params"].double()
    mean = zf.sum(1) / n
    var = ((zf * zf).sum(1) / n - mean * mean).clamp_min(0)
    sc = P[0] / torch.sqrt(var + NT.BN_EPS)
    out = {"mean": mean, "var": var, "scale": sc, "shift": P[1] - mean * sc}
    m = float(torch.tensor(c.momentum, dtype=torch.float32))
    if c.update:
        out["running_mean"] = (1 - m) * P[2] + m * mean
        out["running_var"] = (1 - m) * P[3] + m * var * (n / (n - 1.0))
    return {k: v.float().double() for k, v in out.items()}


def _stats_key(k):
    return "bn_running" if k.startswith("running") else "bn_stats"


def test_batchnorm_statistics_restatement_and_mutants():
    caught = {"border": 0, "n": 0, "drop": 0, "double": 0}
    for c in NT.STATS_CASES:
        d = NT.stats_inputs(c.name)
        ref = NT.stats_reference(c, d)
        for k, y in _stats_one_pass(c, d).items():
            assert NT.measure(y, *ref[k]) <= NT.bar(_stats_key(k)), (c.name, k)
        assert float(ref["var"][0][1]) == 0.0
        n = c.B * c.h * c.w
        muts = {"border": NT.stats_reference(c, d, border_cell=3.0), "drop": NT.stats_reference(c, d, drop_pixel=(n - 1) // NT.BN_PIECE * NT.BN_PIECE),
                "double": NT.stats_reference(c, d, double_pixel=max(0, (n - 1) // NT.BN_PIECE * NT.BN_PIECE - 1))}
        if c.update:
            muts["n"] = NT.stats_reference(c, d, n_for_n1=True)
        for name, mut in muts.items():
            keys = ("running_var",) if name == "n" else ("mean", "var")
            for k in keys:
                assert NT.measure(mut[k][0], *ref[k]) > NT.bar(_stats_key(k)), (c.name, name, k)
            caught[name] += 1
    assert min(caught.values()) >= 3


def test_batchnorm_apply_emulation():
    for c in NT.APPLY_CASES:
        d = NT.apply_inputs(c.name)
        ref, den = NT.apply_reference(c, d)["out"]
        assert NT.measure(NT.apply_reference(c, d, emulate=True), ref, den) <= NT.bar("bn_apply"), c.name
        # a summand left out, the residual left out: far outside the bar
        for drop in ("z1", "res"):
            if drop in d:
                less = {k: v for k, v in d.items() if k != drop}
                assert NT.measure(NT.apply_reference(c, less)["out"][0], ref, den) > 1e3 * NT.bar("bn_apply"), (c.name, drop)


def test_batchnorm_backward_emulation_and_mutants():
    flips = means = 0
    for c in NT.BWD_CASES:
        d = NT.bwd_inputs(c.name)
        ref, emu = NT.bwd_reference(c, d), NT.bwd_emulate(c, d)
        for k, y in emu.items():
            ok = ref[k][0].abs() < 0.99 * NT.RANGE_LIMIT
            assert NT.measure(y[ok], ref[k][0][ok], ref[k][1][ok]) <= NT.bar("bn_bwd_dz"), (c.name, k)
        if c.trip:
            continue
        # one mask bit flipped (an element the mask passes is dropped; one it drops is passed)
        on = int(torch.nonzero(NT.bwd_mask(d).view(-1))[3])
        for idx in (on, 1):
            mut = NT.bwd_reference(c, d, flip=idx)
            assert not torch.equal(mut["dy_out"][0], ref["dy_out"][0])
            assert NT.measure(mut["dz0"][0], *ref["dz0"]) > NT.bar("bn_bwd_dz"), (c.name, idx)
            assert NT.measure(mut["dbias0"][0], *ref["dbias0"]) > NT.bar("bn_bwd_sums"), (c.name, idx)
            assert NT.measure(mut["coef0"][0], *ref["coef0"]) > NT.bar("bn_bwd_sums"), (c.name, idx)
            flips += 1
        if c.two:      # l1's mean used for l0
            mut = NT.bwd_reference(c, d, mean_from=1)
            assert NT.measure(mut["dweight0"][0], *ref["dweight0"]) > NT.bar("bn_bwd_sums"), c.name
            means += 1
    assert flips >= 10 and means >= 3


def test_weight_gradient_emulation_and_mutants():
    by = NT.WG_CASE_BY_NAME
    for c in NT.WGRAD_CASES:
        if c.cout > 64:
            continue                          # (the large cases' emulations run once, in emulation_maxima)
        d = NT.wgrad_inputs(c.name)
        ref, emu = NT.wgrad_reference(c, d), NT.wgrad_emulate(c, d)
        for k, y in emu.items():
            assert NT.measure(y, *ref[k]) <= NT.bar(NT.WG_KEYS[k]), (c.name, k)
    bar = NT.bar("wgrad")
    # a pixel dropped at a piece boundary, and one doubled (the last pixel of piece 0 / the first of piece 1)
    for name in ("plain_k0_32x32_1x12x13", "plain_k1_32x32_1x14x16", "plain_k2_32x32_1x12x13", "plain_k0_64x64_3x6x10"):
        c, d = by[name], NT.wgrad_inputs(name)
        ref, den = NT.wgrad_reference(c, d)["dw"]
        pieces, cpp = NT.wgrad_pieces(c.cout, c.K, c.B, c.h, c.w)
        assert pieces >= 2
        edge = cpp * NT.WG_KC
        for pix, f in ((edge, 0.0), (edge - 1, 0.0), (edge, 2.0), (edge - 1, 2.0)):
            if float(d["gv"][pix // (c.h * c.w)]) != 0.0:
                assert NT.measure(NT.wgrad_reference(c, d, pixel_scale=(pix, f))["dw"][0], ref, den) > bar, (name, pix, f)
    # one chunk's pixels weighted with the neighbouring image's gv: 6 x 10 images, chunk 1 = pixels 32 .. 63 straddles images 0 and 1
    for name in ("plain_k0_64x64_3x6x10", "plain_k1_64x64_3x6x10", "plain_k2_64x64_3x6x10"):
        c, d = by[name], NT.wgrad_inputs(name)
        ref, den = NT.wgrad_reference(c, d)["dw"]
        assert NT.measure(NT.wgrad_reference(c, d, gv_swap=(60, 64, 0))["dw"][0], ref, den) > bar, name
        assert NT.measure(NT.wgrad_reference(c, d, gv_swap=(120, 128, 1))["dw"][0], ref, den) > bar, name
    # one tap shifted by a pixel; the kind-1 phase / tap map with dy and dx swapped
    for name, tap in (("plain_k0_32x32_2x5x7", 0), ("plain_k0_32x32_2x5x7", 4), ("plain_k1_32x32_2x5x7", 5), ("plain_k1_64x64_3x6x10", 1)):
        c, d = by[name], NT.wgrad_inputs(name)
        ref, den = NT.wgrad_reference(c, d)["dw"]
        mut = NT.wgrad_reference(c, d, tap_shift=tap)["dw"][0]
        assert NT.measure(mut, ref, den) > bar, (name, tap)
        others = [t for t in range(9) if t != tap]
        assert torch.equal(mut.view(c.cout, c.cin, 9)[..., others], ref.view(c.cout, c.cin, 9)[..., others])       # one tap only
    for name in ("plain_k1_32x32_2x5x7", "plain_k1_64x64_3x6x10"):
        c, d = by[name], NT.wgrad_inputs(name)
        ref, den = NT.wgrad_reference(c, d)["dw"]
        assert NT.measure(NT.wgrad_reference(c, d, swap=True)["dw"][0], ref, den) > bar, name
    # one weight-norm row using the wrong g
    for name in ("wn_k0_32x32_2x5x7", "wn_k1_64x64_3x6x10", "wn_k2_32x32_1x12x13"):
        c, d = by[name], NT.wgrad_inputs(name)
        ref, mut = NT.wgrad_reference(c, d), NT.wgrad_reference(c, d, wrong_g_row=5)
        e = (mut["dv"][0] - ref["dv"][0]).abs() / ref["dv"][1]
        assert float(e[5].max()) > NT.bar("wgrad_wn_v") and float(e[:5].max()) == 0 and float(e[6:].max()) == 0, name
        assert NT.measure(mut["dg"][0], *ref["dg"]) > NT.bar("wgrad_wn_g"), name


def test_head_emulation_and_a_wrong_row_mutant():
    for c in NT.HEAD_CASES:
        d = NT.head_inputs(c.name)
        ref, emu = NT.head_reference(c, d), NT.head_emulate(c, d)
        assert NT.measure(emu["gf"], *ref["gf"]) <= NT.bar("head_gf"), c.name
        assert NT.measure(emu["grad"], *ref["grad"]) <= NT.bar("head_param"), c.name
        assert ref["grad"][0].numel() == NT.head_params(c, d).numel()
        # an image's row added twice to the batch sums
        d2 = dict(d, gd=torch.cat([d["gd"], d["gd"][:1]]), gp=torch.cat([d["gp"], d["gp"][:1]]), feat=torch.cat([d["feat"], d["feat"][:1]]))
        mut = NT.head_reference(c._replace(B=c.B + 1), d2)["grad"][0]
        assert NT.measure(mut, *ref["grad"]) > NT.bar("head_param"), c.name


def test_threshold_references_and_seed_restatement():
    for c in NT.DOT_CASES:
        d = NT.dot_inputs(c.name)
        ref, den = NT.dot_reference(c, d)
        assert bool((den > ref.abs()).all())
        if c.resG:       # the residual read with the mask's group count (resG < mG)
            wrong = dict(d, m=d["m"][:, 8 * (c.mG - c.resG):]) if c.mG > c.resG else None
            if wrong:
                assert NT.measure(NT.dot_reference(c, wrong)[0], ref, den) > NT.DOUBLE_BAR
    for c in NT.FC_CASES:
        d = NT.clip_inputs(c.name)
        ref = NT.fc_reference(c, d)
        st = d["act"].double() * NT.ASCALE
        exclusive = ((d["gv"].double().view(-1, 1) * (st < NT.THR).double().sum((2, 3))).sum(0) / (c.h * c.w) * d["fc_w"].double())
        assert NT.measure(exclusive, *ref["a20"]) > NT.DOUBLE_BAR            # a value at the threshold counts as clipped
    c = NT.SEED_BY_NAME["seed_f16_ties"]
    d = NT.seed_inputs(c.name)
    p32 = (d["gf"][0, :NT.SEED_TIES] * (torch.tensor(16.0) / torch.tensor(6.0)))
    p64 = d["gf"][0, :NT.SEED_TIES].double() * float(torch.tensor(16.0) / torch.tensor(6.0))
    assert bool((p32.half().float() != p32).all()) and bool(((p32.abs() * 2 ** 11) % 2 == 1).all())          # f16 ties, every one
    apart = p32.half() != NT.half_of_double(p64)
    assert 16 <= int(apart.sum()) <= NT.SEED_TIES - 16                    # the two conversions round apart on some, together on others
    ref, den = NT.seed_reference(c, d)
    fused = NT.seed_fused_pack(c, d)
    assert NT.measure(fused, ref, den) > 100 * NT.bar("grad_seed")        # the fused pack is 2^-11 off on those ...
    assert NT.measure(fused[0, NT.SEED_TIES:], ref[0, NT.SEED_TIES:], den[0, NT.SEED_TIES:]) <= NT.bar("grad_seed")       # ... and only there
    for c in NT.SEED_CASES:
        d = NT.seed_inputs(c.name)
        slot, gv, ga = NT.seed_restate(c, d)
        m = float(d["gf"].abs().max())
        if m == 0:
            assert slot.tolist() == [0.0, 0.0] and float(ga.abs().max()) == 0
        else:
            assert 0.5 <= m * float(slot[0]) < 1 and float(slot[0]) * float(slot[1]) == 1 and float(gv[0]) * float(slot[0]) * c.boost == 1
