"""The argument contract of the ten fused solver loops (csrc/csmri.hip, csrc/tasks.hip) at the C boundary: which calls are
rejected, with which status and which pnpx_last_error() text; what a T = 0 call returns; what the ops.py wrappers return for an
empty batch.  Almost nothing is launched: a rejected call returns before its first launch, a T = 0 call is one copy.

Every rejected call below is rejected by an explicit check that stands before the entry's first launch, and every expected string
is the literal of that check.  All pointers that a case does not null are real buffers of the full size, also where the case's
point is a bad integer: no case relies on the library reading nothing."""
import ctypes as C

import pytest
import torch

from tfpnp_amd import _lib, ops

pytestmark = pytest.mark.gpu

ERR_ARG = 1          # include/pnpx.h PNPX_ERR_ARG
B, H, W, S, V, TMAX = 2, 16, 32, 2, 8, 2
CSMRI_BAD = "csmri: bad argument (null pointer, B<=0 or param_stride < T)"

# family -> state [B,nvar,...], complex or real, measurement kind, hyper-parameter tensors, and the messages of its checks:
#   bad: the forward loop's argument check;  train: the train entry's saved / ticket check;  bwd: the backward entry's argument
#   check;  bwd_null: the backward's T > 0 pointer check (tasks.hip: one check does both);  neg_T: a train call with T < 0 and a
#   null saved (csmri.hip lets it through to the loop's check, tasks.hip's entries reject it themselves)
FAMILIES = {
    "csmri_admm": dict(nvar=3, cplx=True, aux="csmri", hyper=2, bad=CSMRI_BAD, bwd=CSMRI_BAD, neg_T=CSMRI_BAD,
                       train="csmri_admm_train: saved / ticket is null", bwd_null="csmri_admm_backward: null pointer",
                       null_hyper={}),   # mu / tau: not checked on the host
    "csmri_hqs": dict(nvar=2, cplx=True, aux="csmri", hyper=2, bad=CSMRI_BAD, bwd=CSMRI_BAD, neg_T=CSMRI_BAD,
                      train="csmri_hqs_train: saved / ticket is null", bwd_null="csmri_hqs_backward: null pointer",
                      null_hyper={}),   # mu / tau: not checked on the host
    "csmri_pg": dict(nvar=1, cplx=True, aux="csmri", hyper=2, bad=CSMRI_BAD, bwd=CSMRI_BAD, neg_T=CSMRI_BAD,
                     train="csmri_pg_train: saved / ticket is null", bwd_null="csmri_pg_backward: null pointer",
                     null_hyper={}),   # mu / tau: not checked on the host
    "csmri_apg": dict(nvar=2, cplx=True, aux="csmri", hyper=3, bad=CSMRI_BAD, bwd=CSMRI_BAD, neg_T=CSMRI_BAD,
                      train="csmri_apg_train: saved / ticket is null", bwd_null="csmri_apg_backward: null pointer",
                      null_hyper={"h1": "csmri_apg: null tau/beta", "h2": "csmri_apg: null tau/beta"}),
    "csmri_redadmm": dict(nvar=3, cplx=True, aux="csmri", hyper=3, bad=CSMRI_BAD, bwd=CSMRI_BAD, neg_T=CSMRI_BAD,
                          train="csmri_redadmm_train: saved / ticket is null",
                          bwd_null="csmri_redadmm_backward: null pointer",
                          null_hyper={"h1": "csmri_redadmm: null mu/lamda", "h2": "csmri_redadmm: null mu/lamda"}),
    "pr_iadmm": dict(nvar=3, cplx=True, aux="pr", hyper=3, bad="pnpx_pr_iadmm: bad argument",
                     train="pnpx_pr_iadmm_train: saved / ticket is null", bwd="pnpx_pr_iadmm_backward: bad argument",
                     bad_ints={"S": 0}),
    "pr_pg": dict(nvar=1, cplx=True, aux="pr", hyper=2, bad="pnpx_pr_pg: bad argument",
                  train="pnpx_pr_pg_train: saved / ticket is null", bwd="pnpx_pr_pg_backward: bad argument",
                  bad_ints={"S": 0, "H": 0, "W": 0}),
    "spi_admm": dict(nvar=3, cplx=False, aux="spi", hyper=2, bad="pnpx_spi_admm: bad argument",
                     train="pnpx_spi_admm_train: saved / ticket is null", bwd="pnpx_spi_admm_backward: bad argument"),
    "ct_iadmm": dict(nvar=3, cplx=False, aux="ct", hyper=3, bad="pnpx_ct_iadmm: bad argument",
                     train="pnpx_ct_iadmm_train: saved / ticket is null", bwd="pnpx_ct_iadmm_backward: bad argument",
                     bad_ints={"R": 0, "n_view": 0, "opnorm": 0.0}),
    "ct_pg": dict(nvar=1, cplx=False, aux="ct", hyper=2, bad="pnpx_ct_pg: bad argument",
                  train="pnpx_ct_pg_train: saved / ticket is null", bwd="pnpx_ct_pg_backward: bad argument",
                  bad_ints={"R": 0, "n_view": 0, "opnorm": 0.0}),
}
for _f in FAMILIES.values():   # tasks.hip: every hyper-parameter pointer is in the loop's check, and one message serves all
    _f.setdefault("bwd_null", _f["bwd"])
    _f.setdefault("neg_T", _f["train"])
    _f.setdefault("null_hyper", {f"h{i}": _f["bad"] for i in range(1, _f["hyper"])})
    _f.setdefault("bad_ints", {})


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    return ops.Context(dev())   # no weights: nothing here reaches the denoiser


def _state_shape(f, b=B):
    hw = (H, H) if f["aux"] == "ct" else (H, W)
    return (b, f["nvar"], *hw, 2) if f["cplx"] else (b, f["nvar"], *hw)


def _aux(f, b=B):
    """The measurement arguments of a family as (name, tensor or number) pairs, in the order of the forward entries."""
    r = lambda *s: torch.rand(*s, device=dev())
    if f["aux"] == "csmri":
        return [("y0", r(b, 1, H, W, 2)), ("mask", (r(b, 1, H, W) > 0.5).to(torch.uint8))]
    if f["aux"] == "pr":
        return [("y0", r(b, S, H, W)), ("mask", r(b, S, H, W, 2))]
    if f["aux"] == "spi":
        return [("x0", r(b, 1, H, W)), ("K", r(b, 1, H, W) + 1.0)]
    return [("y0", r(b, 1, V, ops.radon_det_count(H))), ("n_view", V), ("opnorm", 1.0)]


def _dims(f):
    return {"csmri": dict(B=B, H=H, W=W), "pr": dict(B=B, S=S, H=H, W=W), "spi": dict(B=B, H=H, W=W),
            "ct": dict(B=B, R=H)}[f["aux"]]


class Call:
    """The named C arguments of one entry, real buffers throughout; `over` replaces single ones (None = a null pointer)."""

    def __init__(self, name, f, kind, T, ctx, over=()):
        torch.manual_seed(5)
        self.keep = []
        self.state = torch.rand(_state_shape(f), device=dev())
        self.out = torch.full_like(self.state, -7.0)
        hyper = {f"h{i}": torch.rand(B, TMAX, device=dev()) for i in range(f["hyper"])}
        saved = torch.zeros(64 * 1024, device=dev())     # more than any family needs at T <= TMAX: (2S+5) * TMAX * B * H * W
        work = torch.zeros(16 * 1024, device=dev())      # CT iADMM: 6 * B * R * R + 2 * n_view
        a = dict(ctx=ctx.handle)
        if kind == "bwd":
            a.update(_aux(f)[1:] if f["aux"] == "ct" else _aux(f))   # the CT backward entries take no sinogram
            a.update(hyper, stride=TMAX, saved=saved, gout=self.state, gin=self.out)
            a.update({f"g{i}": torch.zeros(TMAX, B, device=dev()) for i in range(f["hyper"])}, work=work)
            a.update(_dims(f), T=T, ticket=0)
        else:
            a.update(vin=self.state, vout=self.out)
            a.update(_aux(f))
            a.update(hyper, stride=TMAX)
            a.update(_dims(f), T=T)
            if kind == "train":
                self.ticket = C.c_ulonglong(77)
                a.update(saved=saved, ticket=C.byref(self.ticket))
        a["stream"] = ops._stream(self.state)
        assert set(over) <= set(a), (set(over) - set(a), name, kind)
        a.update(over)
        self.keep = list(a.values())
        self.fn = getattr(_lib.lib(), "pnpx_" + name + {"fwd": "", "train": "_train", "bwd": "_backward"}[kind])
        self.args = [v.data_ptr() if isinstance(v, torch.Tensor) else v for v in a.values()]

    def __call__(self):
        with torch.cuda.device(dev()):
            return self.fn(*self.args)


def _rejected(name, f, kind, T, ctx, over, msg):
    st = Call(name, f, kind, T, ctx, over)()
    err = _lib.lib().pnpx_last_error().decode()
    print(f"{name} {kind} T={T} {over}: status {st}, {err!r}")
    assert st == ERR_ARG and err == msg, (name, kind, over, st, err, msg)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_rejected_arguments(ctx, name):
    f = FAMILIES[name]
    for kind in ("fwd", "train"):
        _rejected(name, f, kind, 1, ctx, dict(ctx=None), "null context")
        _rejected(name, f, kind, 1, ctx, dict(B=0), f["bad"])
        _rejected(name, f, kind, 1, ctx, dict(T=-1), f["bad"])
        _rejected(name, f, kind, 2, ctx, dict(stride=1), f["bad"])
        _rejected(name, f, kind, 1, ctx, dict(vin=None), f["bad"])
        _rejected(name, f, kind, 1, ctx, dict(vout=None), f["bad"])
        _rejected(name, f, kind, 1, ctx, dict(y0=None) if f["aux"] != "spi" else dict(x0=None), f["bad"])
        _rejected(name, f, kind, 1, ctx, dict(h0=None), f["bad"])
        for h, msg in f["null_hyper"].items():
            _rejected(name, f, kind, 1, ctx, {h: None}, msg)
        for k, v in f["bad_ints"].items():
            _rejected(name, f, kind, 1, ctx, {k: v}, f["bad"])
    _rejected(name, f, "bwd", 1, ctx, dict(ctx=None), "null context")
    _rejected(name, f, "bwd", 1, ctx, dict(B=0), f["bwd"])
    _rejected(name, f, "bwd", 1, ctx, dict(T=-1), f["bwd"])
    _rejected(name, f, "bwd", 2, ctx, dict(stride=1), f["bwd"])
    _rejected(name, f, "bwd", 1, ctx, dict(gout=None), f["bwd"])
    _rejected(name, f, "bwd", 1, ctx, dict(gin=None), f["bwd"])
    _rejected(name, f, "bwd", 1, ctx, dict(h0=None), f["bwd"])
    for k in ("saved", "work", "g0", "g1"):
        _rejected(name, f, "bwd", 1, ctx, {k: None}, f["bwd_null"])
    for k, v in f["bad_ints"].items():
        _rejected(name, f, "bwd", 1, ctx, {k: v}, f["bwd"])


@pytest.mark.parametrize("name", list(FAMILIES))
def test_train_entry_needs_saved_and_ticket(ctx, name):
    f = FAMILIES[name]
    _rejected(name, f, "train", 1, ctx, dict(ticket=None), f["train"])
    _rejected(name, f, "train", 0, ctx, dict(ticket=None), f["train"])
    _rejected(name, f, "train", 1, ctx, dict(saved=None), f["train"])
    _rejected(name, f, "train", 1, ctx, dict(saved=None, ticket=None), f["train"])
    _rejected(name, f, "train", -1, ctx, dict(saved=None), f["neg_T"])


def test_amp_rejected_arguments(ctx):
    f = dict(nvar=2, cplx=True, aux="csmri", hyper=2)   # h1 stands for the probe [T,B,1,H,W]: B * TMAX floats are not read
    for over, msg in ((dict(ctx=None), "null context"), (dict(B=0), CSMRI_BAD), (dict(T=-1), CSMRI_BAD),
                      (dict(vout=None), CSMRI_BAD), (dict(h0=None), CSMRI_BAD), (dict(h1=None), "csmri_amp: probe is null")):
        _rejected("csmri_amp", f, "fwd", 1, ctx, over, msg)
    _rejected("csmri_amp", f, "fwd", 2, ctx, dict(stride=1), CSMRI_BAD)


@pytest.mark.parametrize("name", list(FAMILIES) + ["csmri_amp"])
def test_zero_iterations_pass_the_state_through(ctx, name):
    f = FAMILIES.get(name) or dict(nvar=2, cplx=True, aux="csmri", hyper=2)
    for kind in ("fwd", "train", "bwd") if name in FAMILIES else ("fwd",):
        # train: a null saved is allowed at T = 0 (the entry's own check says so); everything else stays a real buffer
        c = Call(name, f, kind, 0, ctx, dict(saved=None) if kind == "train" else {})
        st = c()
        torch.cuda.synchronize()
        assert st == 0, (name, kind, st, _lib.lib().pnpx_last_error())
        assert c.out.dtype == c.state.dtype and torch.equal(c.out.view(torch.int32), c.state.view(torch.int32)), (name, kind)
        if kind == "train":
            assert c.ticket.value == 0, (name, c.ticket.value)


def _empty_inputs(name, f, T=3):
    e = lambda *s: torch.empty(*s, device=dev())
    v = e(_state_shape(f, 0))
    aux = [a for _, a in _aux(f, 0)]
    if f["aux"] == "csmri":
        aux[1] = aux[1].bool()
    return v, aux, [e(0, T) for _ in range(f["hyper"])]


@pytest.mark.parametrize("name", list(FAMILIES))
def test_empty_batch_shapes_through_ops(ctx, name):
    f = FAMILIES[name]
    T = 3
    v, aux, hyper = _empty_inputs(name, f, T)
    out = getattr(ops, name)(ctx, v, *aux, *hyper)
    assert isinstance(out, torch.Tensor) and out.shape == v.shape and out.dtype == torch.float32
    out, saved, ticket = getattr(ops, name + "_train")(ctx, v, *aux, *hyper)
    assert out.shape == v.shape and saved.shape == (0,) and saved.dtype == torch.float32 and ticket == 0
    baux = aux[1:] if f["aux"] == "ct" else aux
    res = getattr(ops, name + "_backward")(ctx, *baux, *hyper, saved, v)
    assert isinstance(res, tuple) and len(res) == 1 + f["hyper"]
    assert res[0].shape == v.shape
    assert all(g.shape == (0, T) and g.dtype == torch.float32 and g.is_contiguous() for g in res[1:])
    # iter_num below the columns provided: the same shapes, T columns of gradient become iter_num
    res = getattr(ops, name + "_backward")(ctx, *baux, *hyper, saved, v, 2)
    assert all(g.shape == (0, 2) for g in res[1:])
