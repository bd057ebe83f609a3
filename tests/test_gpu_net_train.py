"""The 16 training kernels of the actor and the critic, one launcher call at a time (pnpx_net_train_probe), against float64 references
(cases, references, emulations and bars: tests/net_train_cases.py; derived bars: profiles/net_train_probe.md).

Per case: the bar, or bit identity with the restatement; input border cells hold finite garbage (the weight gradient's X keeps the zero
padding its contract names); every output pre-filled with a sentinel, so a skipped element shows and a written border cell shows; 1 MiB
of a fixed bit pattern before and after every output untouched; a second call bit-identical."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import net_train_cases as NT
from tests.test_gpu_vjp_glue import PNPX_ERR_ARG, PNPX_ERR_HIP, PNPX_ERR_SHAPE, Slab

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0            # f16-exact; as a record value 77.125
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


def probe(ctx, op, sizes, outs, expect=0, host=None, **operands):
    """One pnpx_net_train_probe call; operands / outs: {descriptor field: Slab}; host: {field: numpy array}.  The outputs' guards are checked."""
    from tfpnp_amd import _lib
    D = _lib.NetTrainProbeDesc(op=op, **sizes)
    for k, v in list(operands.items()) + list(outs.items()):
        setattr(D, k, v.ptr())
    for k, v in (host or {}).items():
        setattr(D, k, v.ctypes.data)
    torch.cuda.synchronize()
    st = _lib.lib().pnpx_net_train_probe(ctx.handle, C.byref(D), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if st == PNPX_ERR_HIP:                 # a HIP runtime error: nothing more may be started on this device
        pytest.exit("pnpx_net_train_probe: " + _lib.lib().pnpx_last_error().decode(), returncode=3)
    torch.cuda.synchronize()
    assert st == expect, (st, _lib.lib().pnpx_last_error().decode())
    for k, v in outs.items():
        assert v.guards_intact(), f"the launch wrote outside its output {k}"
    return st


def rec_in(x, garbage=None):
    return Slab(NT.records(x, garbage=garbage))


def rec_out(B, Cn, h, w):
    return Slab(torch.full((B, Cn // 8, h + 2, w + 2, 16), SENTINEL, dtype=torch.float16))


def f32_out(*shape):
    return Slab(torch.full(shape, NAN))


def interior(slab, what, border=SENTINEL):
    """The interior records of an output on the CPU; every border record still holds `border`."""
    t = slab.cpu()
    b = t.clone()
    b[:, :, 1:-1, 1:-1] = border
    assert bool((b == border).all()), f"{what}: a border record of the output was written"
    r = t[:, :, 1:-1, 1:-1].contiguous()
    assert bool(torch.isfinite(r.float()).all()) or what.endswith("(range)"), f"{what}: a record is not finite"
    return r


def report(key, name, e, b, what=""):
    print(f"\nnet_train_probe {key} {name} {what} measure {e:.4e} bar {b:.4e}")
    assert e <= b, (key, name, what, e, b)


def twice(run):
    """run() -> tuple of CPU tensors; a second call gives the same bits."""
    first, again = run(), run()
    for a, b in zip(first, again):
        assert NT.bits_equal(a, b) if a.dtype in (torch.float32, torch.float16) else torch.equal(a, b), "second call differs"
    return first


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm

@pytest.mark.parametrize("case", NT.STATS_CASES, ids=lambda c: c.name)
def test_bn_stats(ctx, case):
    c, d = case, NT.stats_inputs(case.name)
    Cn = 8 * c.G
    z = rec_in(d["z0"], garbage=c.name)

    def run():
        params, fout = Slab(d["params"].reshape(-1)), f32_out(4 * Cn)
        probe(ctx, NT.BN_STATS, dict(B=c.B, G=c.G, h=c.h, w=c.w, momentum=c.momentum, update=c.update), {"fout": fout, "params": params}, z0=z)
        return fout.cpu().view(4, Cn), params.cpu().view(4, Cn)
    got, P = twice(run)
    ref = NT.stats_reference(c, d)
    for i, k in enumerate(("mean", "var", "scale", "shift")):
        report("bn_stats", c.name, NT.measure(got[i], *ref[k]), NT.bar("bn_stats"), k)
    assert NT.bits_equal(P[:2].contiguous(), d["params"][:2].contiguous()), "weight or bias changed"
    if c.update:
        for i, k in ((2, "running_mean"), (3, "running_var")):
            report("bn_running", c.name, NT.measure(P[i], *ref[k]), NT.bar("bn_running"), k)
    else:
        assert NT.bits_equal(P, d["params"]), "running statistics moved without the update flag"


def _unshuffle(s2d_rec, G):
    """Interior records of a space-to-depth copy [B][4 G][h/2][w/2][16] -> [B][G][h][w][16]."""
    B, G4, h2, w2, _ = s2d_rec.shape
    out = torch.empty(B, G, 2 * h2, 2 * w2, 16, dtype=s2d_rec.dtype)
    for py in (0, 1):
        for px in (0, 1):
            out[:, :, py::2, px::2] = s2d_rec[:, (2 * py + px) * G:(2 * py + px + 1) * G]
    return out


@pytest.mark.parametrize("case", NT.APPLY_CASES, ids=lambda c: c.name)
def test_bn_apply(ctx, case):
    c, d = case, NT.apply_inputs(case.name)
    Cn = 8 * c.G
    ops = {"z0": rec_in(d["z0"], garbage=c.name + "a"), "st0": Slab(d["st0"].reshape(-1))}
    if c.two:
        ops.update(z1=rec_in(d["z1"], garbage=c.name + "b"), st1=Slab(d["st1"].reshape(-1)))
    if c.res:
        ops["res"] = rec_in(d["res"], garbage=c.name + "r")

    def run():
        outs = {}
        if c.out:
            outs["out"] = rec_out(c.B, Cn, c.h, c.w)
        if c.s2d:
            outs["out2"] = rec_out(c.B, 4 * Cn, c.h // 2, c.w // 2)
        probe(ctx, NT.BN_APPLY, dict(B=c.B, G=c.G, h=c.h, w=c.w), outs, **ops)
        return tuple(interior(outs[k], c.name + " " + k) for k in ("out", "out2") if k in outs)
    got = twice(run)
    rec = got[0] if c.out else _unshuffle(got[0], c.G)
    if c.out and c.s2d:
        assert NT.bits_equal(_unshuffle(got[1], c.G), got[0]), "the space-to-depth copy differs from out"
    ref, den = NT.apply_reference(c, d)["out"]
    report("bn_apply", c.name, NT.measure(NT.decode_interior(rec), ref, den), NT.bar("bn_apply"))


@pytest.mark.parametrize("case", NT.BWD_CASES, ids=lambda c: c.name)
def test_bn_bwd(ctx, case):
    c, d = case, NT.bwd_inputs(case.name)
    Cn, nl = 8 * c.G, 2 if c.two else 1
    ops = {"g": rec_in(d["g"], garbage=c.name + "g"), "act": rec_in(d["act"], garbage=c.name + "a"), "z0": rec_in(d["z0"], garbage=c.name + "z"),
           "st0": Slab(d["st0"].reshape(-1)), "params": Slab(d["params"].reshape(-1))}
    if c.two:
        ops.update(z1=rec_in(d["z1"], garbage=c.name + "y"), st1=Slab(d["st1"].reshape(-1)))
    if c.slot:
        ops["slot"] = Slab(torch.tensor(c.slot, dtype=torch.float32))

    def run():
        outs = {"grad": f32_out(nl * 4 * Cn), "coef": f32_out(nl * 3 * Cn), "out": rec_out(c.B, Cn, c.h, c.w), "flag": Slab(torch.zeros(1, dtype=torch.int32))}
        if c.two:
            outs["out2"] = rec_out(c.B, Cn, c.h, c.w)
        if c.dy_out:
            outs["dy_out"] = rec_out(c.B, Cn, c.h, c.w)
        probe(ctx, NT.BN_BWD, dict(B=c.B, G=c.G, h=c.h, w=c.w, boost=c.boost), outs, **ops)
        tag = " (range)" if c.trip else ""
        return (outs["grad"].cpu().view(nl, 4, Cn), outs["coef"].cpu().view(nl, 3, Cn), outs["flag"].cpu()) + tuple(
            interior(outs[k], c.name + " " + k + tag) for k in ("out", "out2", "dy_out") if k in outs)
    got = twice(run)
    grad, coef, flag, dz = got[0], got[1], got[2], got[3:3 + nl]
    ref = NT.bwd_reference(c, d)
    assert NT.bits_equal(d["params"].reshape(-1), ops["params"].cpu()), "the parameters changed"
    assert int(flag[0]) == (1 if c.trip else 0), "range flag"
    for i in range(nl):
        r, den = ref["dz%d" % i]
        ok = r.abs() < 0.99 * NT.RANGE_LIMIT
        report("bn_bwd_dz", c.name, NT.measure(NT.decode_interior(dz[i])[ok], r[ok], den[ok]), NT.bar("bn_bwd_dz"), "dz%d" % i)
        report("bn_bwd_sums", c.name, NT.measure(grad[i, 0], *ref["dweight%d" % i]), NT.bar("bn_bwd_sums"), "dweight%d" % i)
        report("bn_bwd_sums", c.name, NT.measure(grad[i, 1], *ref["dbias%d" % i]), NT.bar("bn_bwd_sums"), "dbias%d" % i)
        report("bn_bwd_sums", c.name, NT.measure(coef[i], *ref["coef%d" % i]), NT.bar("bn_bwd_sums"), "coef%d" % i)
        assert NT.bits_equal(grad[i, 2:].contiguous(), torch.zeros(2, Cn)), "the running-statistics slots of the gradient are not +0.0"
    if c.dy_out:
        want = NT.interior_records(torch.where(d["act"] > 0, d["g"], torch.zeros(())))
        assert NT.bits_equal(got[-1], want), "dy_out is not the masked gradient's records"


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradients

@pytest.mark.parametrize("case", NT.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad(ctx, case):
    c, d = case, NT.wgrad_inputs(case.name)
    fan = NT.wg_fan(c)
    ops = {"g": rec_in(d["G"], garbage=c.name), "x": rec_in(d["X"]), "gv": Slab(d["gv"])}
    sizes = dict(B=c.B, h=c.h, w=c.w, cout=c.cout, K=c.K, cin=c.cin, Cp=c.Cp, kind=c.kind, Gg=c.Gg, Xg=c.Xg, inv_w=NT.WG_INV_W)
    if c.wn:
        ops["params"] = Slab(torch.cat([d["bias"], d["wg"], d["v"].reshape(-1)]))
        sizes["inv_b"] = NT.WG_INV_B

    def run():
        grad = f32_out((2 * c.cout if c.wn else 0) + c.cout * fan)
        probe(ctx, NT.WGRAD_WN if c.wn else NT.WGRAD_PLAIN, sizes, {"grad": grad}, **ops)
        return (grad.cpu(),)
    (grad,) = twice(run)
    ref = NT.wgrad_reference(c, d)
    if c.wn:
        got = {"db": grad[:c.cout], "dg": grad[c.cout:2 * c.cout], "dv": grad[2 * c.cout:].view(c.cout, fan)}
    else:
        got = {"dw": grad.view(c.cout, fan)}
    for k, y in got.items():
        report(NT.WG_KEYS[k], c.name, NT.measure(y, *ref[k]), NT.bar(NT.WG_KEYS[k]), k)


# ---------------------------------------------------------------------------------------------------------------------------------
# critic thresholds

@pytest.mark.parametrize("case", NT.CLIP_CASES, ids=lambda c: c.name)
def test_clip_mask(ctx, case):
    c, d = case, NT.clip_inputs(case.name)
    act = rec_in(d["act"], garbage=c.name)

    def run():
        out = rec_out(c.B, 8 * c.G, c.h, c.w)
        probe(ctx, NT.CLIP_MASK, dict(B=c.B, G=c.G, h=c.h, w=c.w, thr=NT.THR), {"out": out}, act=act)
        return (interior(out, c.name, border=0.0),)          # the whole padded tensor is written: a zero border
    (got,) = twice(run)
    want = NT.clip_restate(d)
    assert NT.bits_equal(got, want), c.name
    assert 0 < int((want[..., :8] != 0).sum()) < want[..., :8].numel()


@pytest.mark.parametrize("case", NT.DOT_CASES, ids=lambda c: c.name)
def test_alpha_dot(ctx, case):
    c, d = case, NT.dot_inputs(case.name)
    ops = {"g": rec_in(d["g"], garbage=c.name + "g"), "x": rec_in(d["wm"], garbage=c.name + "w")}
    if c.resG:
        ops.update(res=rec_in(d["res"], garbage=c.name + "r"), m=rec_in(d["m"], garbage=c.name + "m"))

    def run():
        out = Slab(torch.full((c.B,), NAN, dtype=torch.float64))
        probe(ctx, NT.ALPHA_DOT, dict(B=c.B, G=c.G, h=c.h, w=c.w, resG=c.resG, mG=c.mG), {"dout": out}, **ops)
        return (out.cpu(),)
    (got,) = twice(run)
    report("double_out", c.name, NT.measure(got, *NT.dot_reference(c, d)), NT.DOUBLE_BAR)


@pytest.mark.parametrize("case", NT.FC_CASES, ids=lambda c: c.name)
def test_fc_grad(ctx, case):
    c, d = case, NT.clip_inputs(case.name)
    ops = {"act": rec_in(d["act"], garbage=c.name), "gv": Slab(d["gv"]), "fin": Slab(d["fc_w"])}

    def run():
        fout, dout = f32_out(512), Slab(torch.full((512,), NAN, dtype=torch.float64))
        probe(ctx, NT.FC_GRAD, dict(B=c.B, h=c.h, w=c.w, thr=NT.THR), {"fout": fout, "dout": dout}, **ops)
        return fout.cpu(), dout.cpu()
    fcw, a20 = twice(run)
    ref = NT.fc_reference(c, d)
    report("fc_grad", c.name, NT.measure(fcw, *ref["grad_fcw"]), NT.bar("fc_grad"))
    report("double_out", c.name, NT.measure(a20, *ref["a20"]), NT.DOUBLE_BAR, "a20")


@pytest.mark.parametrize("case", NT.FIN_CASES, ids=lambda c: c.name)
def test_alpha_finish(ctx, case):
    c, d = case, NT.fin_inputs(case.name)
    ops = {"din": Slab(d["dots"]), "din2": Slab(d["a20"]), "gv": Slab(d["gv"])}
    src = np.asarray(d["alpha_src"], np.int32)

    def run():
        grad = Slab(torch.full((23,), SENTINEL))
        probe(ctx, NT.ALPHA_FINISH, dict(B=c.B, inv_w=NT.FIN_INV), {"grad": grad}, host={"alpha_src": src}, **ops)
        return (grad.cpu(),)
    (got,) = twice(run)
    ref = NT.fin_reference(c, d)
    worst = 0.0
    for i in range(23):
        if i in ref:
            worst = max(worst, NT.measure(got[i:i + 1], torch.tensor([ref[i][0]], dtype=torch.float64), torch.tensor([ref[i][1]], dtype=torch.float64)))
        else:
            assert float(got[i]) == SENTINEL, f"gradient {i}, which no threshold names, was written"
    report("alpha_finish", c.name, worst, NT.bar("alpha_finish"))


# ---------------------------------------------------------------------------------------------------------------------------------
# actor heads

@pytest.mark.parametrize("case", NT.HEAD_CASES, ids=lambda c: c.name)
def test_head_grad(ctx, case):
    c, d = case, NT.head_inputs(case.name)
    P = NT.head_params(c, d)
    ops = {"act": rec_in(d["feat"], garbage=c.name), "params": Slab(P), "fin": Slab(d["gp"]), "fin2": Slab(d["gd"])}

    def run():
        gf, grad = f32_out(c.B, 512), f32_out(P.numel())
        probe(ctx, NT.HEAD_GRAD, dict(B=c.B, h=c.h, w=c.w, n_det=c.n_det, spi=c.spi), {"fout": gf, "grad": grad}, **ops)
        return gf.cpu(), grad.cpu()
    gf, grad = twice(run)
    ref = NT.head_reference(c, d)
    report("head_gf", c.name, NT.measure(gf, *ref["gf"]), NT.bar("head_gf"))
    report("head_param", c.name, NT.measure(grad, *ref["grad"]), NT.bar("head_param"))


@pytest.mark.parametrize("case", NT.SEED_CASES, ids=lambda c: c.name)
def test_grad_seed(ctx, case):
    c, d = case, NT.seed_inputs(case.name)
    gf = Slab(d["gf"])

    def run():
        slot, gv, ga = f32_out(2), f32_out(c.B), rec_out(c.B, 512, c.h, c.w)
        probe(ctx, NT.GRAD_SEED, dict(B=c.B, h=c.h, w=c.w, boost=c.boost), {"fout": slot, "fout2": gv, "out": ga}, fin=gf)
        return slot.cpu(), gv.cpu(), interior(ga, c.name)
    slot, gv, ga = twice(run)
    want_slot, want_gv, _ = NT.seed_restate(c, d)
    assert NT.bits_equal(slot, want_slot) and NT.bits_equal(gv, want_gv), (slot, gv)
    y = NT.decode_interior(ga)
    if c.kind == "zero":
        assert bool((y == 0).all())
    report("grad_seed", c.name, NT.measure(y, *NT.seed_reference(c, d)), NT.bar("grad_seed"))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals

def test_misplaced_and_missing_operands_are_refused(ctx):
    c = NT.APPLY_CASES[0]
    d = NT.apply_inputs(c.name)
    z, st, out = rec_in(d["z0"]), Slab(d["st0"].reshape(-1)), rec_out(c.B, 8 * c.G, c.h, c.w)
    before = out.cpu()
    sizes = dict(B=c.B, G=c.G, h=c.h, w=c.w)
    probe(ctx, NT.BN_APPLY, sizes, {"out": out}, expect=PNPX_ERR_ARG, z0=z)                          # st0 missing
    probe(ctx, NT.BN_APPLY, sizes, {"out": out}, expect=PNPX_ERR_ARG, z0=z, st0=st, z1=z)            # half a second summand
    probe(ctx, NT.BN_APPLY, sizes, {"out": out}, expect=PNPX_ERR_ARG, z0=z, st0=st, gv=st)           # an operand of another op
    probe(ctx, NT.BN_APPLY, sizes, {}, expect=PNPX_ERR_ARG, z0=z, st0=st)                            # no output
    probe(ctx, NT.BN_APPLY, dict(sizes, h=3), {"out2": out}, expect=PNPX_ERR_SHAPE, z0=z, st0=st)    # space-to-depth of an odd height
    probe(ctx, NT.BN_APPLY, dict(sizes, boost=2.0), {"out": out}, expect=PNPX_ERR_ARG, z0=z, st0=st)
    probe(ctx, NT.BN_BWD, sizes, {"out": out}, expect=PNPX_ERR_ARG, z0=z, st0=st)
    probe(ctx, NT.CLIP_MASK, sizes, {"out": out}, expect=PNPX_ERR_ARG, z0=z)
    probe(ctx, NT.ALPHA_DOT, dict(sizes, resG=1, mG=1), {"dout": out}, expect=PNPX_ERR_ARG, g=z, x=z)     # resG without res / m
    probe(ctx, NT.ALPHA_FINISH, dict(B=2, inv_w=1.0), {"grad": out}, expect=PNPX_ERR_ARG, host={"alpha_src": np.full(21, 21, np.int32)}, din=z, din2=z, gv=st)
    probe(ctx, 11, sizes, {"out": out}, expect=PNPX_ERR_ARG, z0=z, st0=st)
    assert NT.bits_equal(out.cpu(), before), "a refused call wrote its output"
