"""Seeded dump of the DRUNet denoiser for an A/B of two trees (bit-identity of a refactor of csrc/drunet*.hip): forward, pre-clamp
forward and VJP in both kernel families, the SPI ADMM training loop through the DRUNet prox, and Context.bytes() along a call
sequence that re-lays the arenas.  Uses only public names of tfpnp_amd and fixed seeds.  GPU box only.

  dump_drunet.py OUT.npz            run from the tree under test (its own library and Python layer); writes every array
  dump_drunet.py --compare A B      table per case, "N of N arrays np.array_equal", the sensitivity line, RESULT

Cases: conv_mode 0 (m0) and 1 (m1) at (B, H, W) = (2, 16, 24), (3, 32, 32), (5, 64, 64), (1, 256, 256): out, pre, grad_x,
grad_sigma.  conv_mode 1 again with option chains = 1 / 2 / 3, with drunet_shift = 4 and with range_guard = 2.  Per mode one
spi_admm_train + spi_admm_backward at B=2 64x64, T=3, and the bytes() array of the sequence inference B=3 16x24, VJP B=2,
inference B=1, inference B=3, inference B=2 24x16, VJP B=2 16x24, VJP B=1 (the sequence of tests/test_gpu_drunet_arena.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = ((2, 16, 24), (3, 32, 32), (5, 64, 64), (1, 256, 256))
VARIANTS = (("m0", 0, ()), ("m1", 1, ()), ("m1_chains1", 1, (("chains", 1),)), ("m1_chains2", 1, (("chains", 2),)),
            ("m1_chains3", 1, (("chains", 3),)), ("m1_shift4", 1, (("drunet_shift", 4),)), ("m1_guard2", 1, (("range_guard", 2),)))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
    rows = {}
    for k in sorted(a.files):
        x, y = a[k], b[k]
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) and x.tobytes() == y.tobytes()
        r = rows.setdefault(k.rsplit("/", 1)[0], [0, 0, 0])
        r[0] += 1
        r[1] += bool(same)
        r[2] += x.size
        if not same:
            print("DIFFERS:", k, x.dtype, x.shape, y.dtype, y.shape)
    print(f"{'case':32s}{'arrays':>8s}{'bit-identical':>15s}{'elements':>12s}")
    for c, (n, ok, el) in rows.items():
        print(f"{c:32s}{n:8d}{ok:15d}{el:12d}")
    n, ok = sum(r[0] for r in rows.values()), sum(r[1] for r in rows.values())
    print(f"total: {ok} of {n} arrays np.array_equal (and equal bytes, dtype, shape) between {pa} and {pb}")
    for m in ("m0", "m1"):
        print(f"Context.bytes() along the arena sequence, {m}: {a[m + '/arena_sequence/bytes'].tolist()} vs {b[m + '/arena_sequence/bytes'].tolist()}")
    for B, H, W in SHAPES:   # the comparison can fail: within B, a pass scaled by 2^-4 gives other bits than the unscaled one
        k = f"m1_chains1/{B}x{H}x{W}/pre"
        differ = not np.array_equal(b[k], b[k.replace("m1_chains1", "m1_shift4")])
        print(f"sensitivity ({pb}): {k} vs drunet_shift=4: {'differ' if differ else 'EQUAL'}")
    print("RESULT:", "BIT-IDENTICAL" if ok == n else "DIFFERENT")
    return 0 if ok == n else 1


def main(out_path):
    import torch
    from tfpnp_amd import ops, synth
    from tfpnp_amd.pnp import DRUNetDenoiser2D
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    params = synth.make_drunet_params(0)
    out = {}

    def keep(key, v):
        out[key] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    def inputs(B, H, W, seed):
        rs = np.random.RandomState(seed)
        sigma = rs.uniform(5, 50, B).astype(np.float32) / 255.0
        x = synth.phantom_batch(B, H, W, seed).astype(np.float32) + rs.standard_normal((B, 1, H, W)).astype(np.float32) * sigma[:, None, None, None]
        return t(x.astype(np.float32)), t(sigma), t(rs.standard_normal((B, 1, H, W)).astype(np.float32))

    def vjp(den, x, s, g):
        lx, ls = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
        (den(lx, ls) * g).sum().backward()
        return lx.grad, ls.grad

    for tag, mode, options in VARIANTS:
        den = DRUNetDenoiser2D(state_dict=params, conv_mode=mode)
        ctx = den.context(dev)
        for key, value in options:
            ctx.set_option(key, value)
        for i, (B, H, W) in enumerate(SHAPES):
            x, s, g = inputs(B, H, W, 300 + i)
            k = f"{tag}/{B}x{H}x{W}/"
            with torch.no_grad():
                keep(k + "out", den(x, s))
                keep(k + "pre", den.forward_preclamp(x, s)[1])
            gx, gs = vjp(den, x, s, g)
            keep(k + "grad_x", gx)
            keep(k + "grad_sigma", gs)
            print(k, flush=True)
        ctx.status()
        ctx.close()

    for tag, mode in (("m0", 0), ("m1", 1)):
        ctx = ops.Context(dev)
        ctx.load_drunet(params)
        ctx.set_option("conv_mode", mode)
        B, H, W, seed, T = 2, 64, 64, 71, 3          # the case of tests/golden_inputs.py::drunet_spi_case
        d = synth.make_spi_batch(B, H, W, K=6, seed=seed)
        rs = np.random.RandomState(seed + 1)
        sg = t(rs.uniform(15 / 255.0, 70 / 255.0, (B, T)).astype(np.float32))
        mu = t(rs.uniform(50, 120, (B, T)).astype(np.float32))
        x0, K = t(d["x0"]), t(d["K"])
        state = torch.cat([x0, x0, torch.zeros_like(x0)], 1)
        gout = t(rs.standard_normal((B, 3, H, W)).astype(np.float32))
        k = f"{tag}/spi_admm_train/"
        o, saved, ticket = ops.spi_admm_train(ctx, state, x0, K, sg, mu)
        keep(k + "state", o)
        keep(k + "saved", saved)
        for i, gi in enumerate(ops.spi_admm_backward(ctx, x0, K, sg, mu, saved, gout, None, ticket)):
            keep(k + f"g{i}", gi)
        ctx.status()
        ctx.close()
        print(k, flush=True)

        den = DRUNetDenoiser2D(state_dict=params, conv_mode=mode)
        ctx = den.context(dev)
        x3, s3, _ = inputs(3, 16, 24, 401)
        x2, s2, g2 = inputs(2, 16, 24, 402)
        xt, st, _ = inputs(2, 24, 16, 403)
        total = [ctx.bytes()]
        for step in ((x3, s3), (x2, s2, g2), (x3[:1], s3[:1]), (x3, s3), (xt, st), (x2, s2, g2), (x2[:1], s2[:1], g2[:1])):
            if len(step) == 3:
                r = vjp(den, *step)
            else:
                with torch.no_grad():
                    r = (den(*step),)
            for j, v in enumerate(r):
                keep(f"{tag}/arena_sequence/step{len(total)}_{j}", v)
            torch.cuda.synchronize()
            total.append(ctx.bytes())
        keep(f"{tag}/arena_sequence/bytes", np.asarray(total, np.int64))
        ctx.status()
        ctx.close()
        print(f"{tag}/arena_sequence/ bytes {total}", flush=True)
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print(f"wrote {len(out)} arrays, {sum(v.size for v in out.values())} elements, to {out_path}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
