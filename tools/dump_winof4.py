"""Seeded dump of everything the Winograd F(4x4,3x3) kernels of csrc/conv3x3_winof4.hip compute, for an A/B of two builds of the library
(bit-identity of a refactor; PNPX_LIB selects the build, the Python tree is the same).  GPU box only.

  dump_winof4.py OUT.npz            run once per build, each in a fresh process; writes every array
  dump_winof4.py --compare A B      table per group, "N of N arrays np.array_equal", and the sensitivity lines

Single layers (pnpx_conv3x3_probe): kind 4 on the WINOF4 rows of tests/conv_layer_cases.py, kind 8 on tests/winof4_entry_cases.py, kind 11
on tests/winof4_fuse_up_cases.py, kind 12 on tests/winof4_c32_cases.py; the padded output and, where the case has one, the pool output.
Network: unet_denoise's pre-clamp and clamped output at 1x32x64, 2x64x64, 3x64x128 and 6x64x64 under the defaults, under each of
fp32_winof4_layers / _entries / _fuse_up / _c32 at 0 and at all its bits, and -- the K-split claims the decoder entries at these sizes --
with fp32_ksplit 0 under all four at all bits and under each one at 0 beside the other three at all bits; unet_denoise_backward's two
gradients at 3x64x128 under the same settings.  Full size: one forward at 48x256x256 under the defaults, images 0, 5 and 47 and the
float64 sum of every image."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ENTRY_BITS = (1 << 15) | (1 << 18) | (1 << 21)
ALL_BITS = {"fp32_winof4_layers": (1 << 27) - 1, "fp32_winof4_entries": ENTRY_BITS, "fp32_winof4_fuse_up": ENTRY_BITS,
            "fp32_winof4_c32": (1 << 1) | (1 << 2) | (1 << 25)}
SHAPES = ((1, 32, 64), (2, 64, 64), (3, 64, 128), (6, 64, 64))
BWD_SHAPE = (3, 64, 128)
FULL, FULL_KEPT = (48, 256, 256), (0, 5, 47)


def settings():
    """[(tag, {option: value})]; an empty dict = the context's defaults"""
    out = [("defaults", {})]
    for k, v in ALL_BITS.items():
        out += [(f"{k}=0", {k: 0}), (f"{k}=all", {k: v})]
    out.append(("ks0,all", dict(ALL_BITS, fp32_ksplit=0)))
    return out + [(f"ks0,{k}=0", dict(ALL_BITS, fp32_ksplit=0, **{k: 0})) for k in ALL_BITS]


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
    rows = {}
    for k in sorted(a.files):
        x, y = a[k], b[k]
        same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        r = rows.setdefault(k.split("/")[0], [0, 0, 0])
        r[0] += 1
        r[1] += bool(same)
        r[2] += x.size
        if not same:
            print("DIFFERS:", k, x.dtype, x.shape, y.dtype, y.shape)
    print(f"{'group':24s}{'arrays':>8s}{'bit-identical':>15s}{'elements':>12s}")
    for c, (n, ok, el) in rows.items():
        print(f"{c:24s}{n:8d}{ok:15d}{el:12d}")
    n, ok = sum(r[0] for r in rows.values()), sum(r[1] for r in rows.values())
    print(f"total: {ok} of {n} arrays equal by bytes, dtype and shape between {pa} and {pb}")
    # the comparison can fail: within B, an option at 0 and at all its bits gives other bits at the shapes where it moves a layer
    moved = {opt: 0 for opt in ALL_BITS}
    for opt in ALL_BITS:
        for k in sorted(b.files):
            if k.endswith("/pre") and (f"net/{opt}=0/" in k or f"net/ks0,{opt}=0/" in k):
                other = k.replace(f"ks0,{opt}=0/", "ks0,all/").replace(f"{opt}=0/", f"{opt}=all/")
                differ = b[k].tobytes() != b[other].tobytes()
                moved[opt] += differ
                print(f"sensitivity ({pb}): {k} vs {other.split('/')[1]}: {'differ' if differ else 'equal'}")
    # (fp32_winof4_fuse_up is bit-identical to the two-launch form by construction -- tests/test_gpu_winof4_fuse_up.py asserts it -- so its
    # lines read "equal"; its kernel shows in kind 11 and in every ks0 setting)
    sensitive = all(n for opt, n in moved.items() if opt != "fp32_winof4_fuse_up")
    print("sensitivity: shapes at which the option moves the result:", moved, "" if sensitive else "-- AN OPTION MOVES NOTHING")
    print("RESULT:", "DIFFERENT" if ok != n else "BIT-IDENTICAL" if sensitive else "INSENSITIVE")
    return 0 if ok == n and sensitive else 1


def main(out_path):
    import torch
    import torch.nn.functional as F
    from tests import conv_layer_cases as CL
    from tests import winof4_c32_cases as C32
    from tests import winof4_entry_cases as EC
    from tests import winof4_fuse_up_cases as FU
    from tfpnp_amd import _lib, ops, synth
    dev = torch.device("cuda:0")
    out = {}

    def keep(key, v):
        out[key] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    # ---- single layers
    ctx = ops.Context(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def probe(kind, c, d, B, key):
        pad = lambda x: F.pad(x[:B], (CL.PADL, CL.PADL, 1, 1)).to(dev).contiguous()
        in0, in1 = pad(d["in0"]), pad(d["in1"]) if c.C1 else None
        o = torch.zeros(B, c.cout, c.H + 2, c.W + 2 * CL.PADL, device=dev)
        po = torch.zeros(B, c.cout, c.H // 2 + 2, c.W // 2 + 2 * CL.PADL, device=dev) if c.pool else None
        w, bias = d["w"].contiguous().numpy(), d["bias"].contiguous().numpy()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        st = _lib.lib().pnpx_conv3x3_probe(ctx.handle, kind, w.ctypes.data, bias.ctypes.data, c.cout, p(in0), c.C0, p(in1), c.C1, p(o), None, None,
                                           CL.SLOPE, p(po), 1, B, c.H, c.W, stream)
        torch.cuda.synchronize()
        assert st == 0, (key, st, _lib.lib().pnpx_last_error().decode())
        keep(f"kind{kind}/{key}/out", o)
        if po is not None:
            keep(f"kind{kind}/{key}/pool", po)

    for c in CL.CASES:
        if CL.WINOF4 in CL.kinds_of(c) and CL.accepts(CL.WINOF4, c):
            probe(CL.WINOF4, c, CL.inputs(c.name), CL.B_MAX, c.name)
    for i, (_, c) in enumerate(EC.ENTRY_CASES):
        cf, df = EC.full_res(c, EC.inputs(i))
        probe(EC.WINOF4_2SRC, cf, df, EC.B_ALL, c.name)
    for i, (_, c) in enumerate(FU.CASES):
        probe(FU.FUSE_UP, c, FU.inputs(i), EC.B_ALL, c.name)
    for B, c in C32.CASES:
        probe(C32.WINOF4_C32, c, C32.inputs(c.name), B, c.name)
    print("single layers:", len(out), "arrays", flush=True)

    # ---- the network
    params = synth.make_unet_params(0)
    gen = torch.Generator().manual_seed(2604)

    def net_inputs(B, H, W):
        return torch.rand(B, 1, H, W, generator=gen).to(dev), torch.linspace(5 / 255, 50 / 255, B).to(dev)

    cases = {s: net_inputs(*s) for s in SHAPES}
    gout = torch.randn(*BWD_SHAPE[:1], 1, *BWD_SHAPE[1:], generator=gen).to(dev)
    for tag, opts in settings():
        nctx = ops.Context(dev)       # a fresh context per setting: every other option at its default
        nctx.load_unet(params)
        for k, v in opts.items():
            nctx.set_option(k, v)
        for (B, H, W), (x, s) in cases.items():
            o, pre = ops.unet_denoise(nctx, x, s, return_preclamp=True)
            keep(f"net/{tag}/{B}x{H}x{W}/pre", pre)
            keep(f"net/{tag}/{B}x{H}x{W}/out", o)
        x, s = cases[BWD_SHAPE]
        gx, gs = ops.unet_denoise_backward(nctx, x, s, gout)
        keep(f"bwd/{tag}/gx", gx)
        keep(f"bwd/{tag}/gsigma", gs)
        nctx.status()
        print("network:", tag, flush=True)

    # ---- full size
    nctx = ops.Context(dev)
    nctx.load_unet(params)
    x, s = net_inputs(*FULL)
    o, pre = ops.unet_denoise(nctx, x, s, return_preclamp=True)
    for i in FULL_KEPT:
        keep(f"full/image{i}/pre", pre[i])
        keep(f"full/image{i}/out", o[i])
    keep("full/sum_pre", pre.double().sum(dim=(1, 2, 3)))
    keep("full/sum_out", o.double().sum(dim=(1, 2, 3)))
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print(f"wrote {len(out)} arrays, {sum(v.size for v in out.values())} elements, to {out_path} (library {_lib.LIB_PATH})")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
