"""Seeded dump of every fused solver loop for an A/B of two trees (bit-identity of a refactor): forward, train and backward of the
ten loops of tfpnp_amd.ops (CS-MRI ADMM / HQS / PG / APG / RED-ADMM, PR iADMM / PG, SPI ADMM, CT iADMM / PG) and the csmri_amp
forward.  Uses only public names of tfpnp_amd.ops and tfpnp_amd.synth.  GPU box only.

  dump_solver_loops.py OUT.npz            run from the tree under test (its own library and Python layer); writes every array
  dump_solver_loops.py --compare A B      table per case, "N of N arrays np.array_equal", and the sensitivity line

Settings: conv_mode 0 and 1 at B=2 64x64 (generic FFT path) and B=1 256x256 (fast-256 path; PR's fused update of the non-saved path);
conv_mode 1 with range_guard 2 at B=2 64x64 (the re-run wrapper on the path); CT at R=64.  Per case T=3 and iter_num=2 < T;
backward once with the ticket of train and once with ticket 0 (re-computation).  Kept: state, saved, ticket != 0, state gradient,
every hyper-parameter gradient."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

T, ITER, S, N_VIEW = 3, 2, 2, 30


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
    rows = {}
    for k in sorted(a.files):
        x, y = a[k], b[k]
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) and x.tobytes() == y.tobytes()
        r = rows.setdefault(k.rsplit("/", 2)[0], [0, 0, 0])
        r[0] += 1
        r[1] += bool(same)
        r[2] += x.size
        if not same:
            print("DIFFERS:", k, x.dtype, x.shape, y.dtype, y.shape)
    print(f"{'case':44s}{'arrays':>8s}{'bit-identical':>15s}{'elements':>12s}")
    for c, (n, ok, el) in rows.items():
        print(f"{c:44s}{n:8d}{ok:15d}{el:12d}")
    n, ok = sum(r[0] for r in rows.values()), sum(r[1] for r in rows.values())
    print(f"total: {ok} of {n} arrays np.array_equal (and equal bytes, dtype, shape) between {pa} and {pb}")
    for k in sorted(b.files):   # the comparison can fail: within B, T=3 and iter_num=2 give other bits
        if "/T3/" in k and k.endswith("/fwd_state") and "m0/2x64/" in k:
            differ = not np.array_equal(b[k], b[k.replace("/T3/", "/iter2/")])
            print(f"sensitivity ({pb}): {k} vs iter_num={ITER}: {'differ' if differ else 'EQUAL'}")
    print("RESULT:", "BIT-IDENTICAL" if ok == n else "DIFFERENT")
    return 0 if ok == n else 1


def main(out_path):
    import torch
    from tfpnp_amd import ops, synth
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen = torch.Generator().manual_seed(20)
    rn = lambda *s: torch.randn(*s, generator=gen).to(dev)
    params = synth.make_unet_params(0)
    out = {}

    def keep(key, v):
        out[key] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    def hyper(B, lo, hi):
        return t(np.tile(np.linspace(lo, hi, T, dtype=np.float32)[None], (B, 1)))

    def families(ctx, B, H):
        """name -> (state, measurement arguments of the forward, of the backward, hyper-parameters)."""
        sig = hyper(B, 40 / 255, 10 / 255)
        mu, tau, beta, lam = hyper(B, 0.3, 0.7), hyper(B, 0.5, 0.2), hyper(B, 0.2, 0.6), hyper(B, 0.4, 0.8)
        d = synth.make_csmri_batch(B, H, H, seed=3)
        x0, cs = t(d["x0"]), (t(d["y0"]), t(d["mask"]))
        cstate = lambda n: torch.cat([x0] * n, 1) + 0.01 * rn(B, n, H, H, 2)
        p = synth.make_pr_batch(B, H, H, S=S, seed=4)
        pr = (t(p["y0"]), t(p["mask"]))
        pstate = lambda n: torch.cat([torch.stack([t(p["x0"]), torch.zeros_like(t(p["x0"]))], -1)] * n, 1) + 0.01 * rn(B, n, H, H, 2)
        sp = synth.make_spi_batch(B, H, H, seed=5)
        spi = (t(sp["x0"]), t(sp["K"]))
        R = 64
        gt = t(synth.phantom_batch(B, R, R, 6).astype(np.float32))
        y0 = ops.radon_forward(gt, N_VIEW, ctx)
        v = torch.ones_like(gt)
        for _ in range(6):   # operator norm by power iteration on A^T A
            v = ops.radon_backprojection(ops.radon_forward(v, N_VIEW, ctx), R, ctx)
            opnorm = float(v.norm()) ** 0.5
            v = v / v.norm()
        ct = (y0, N_VIEW, opnorm)
        cts = lambda n: torch.cat([0.5 * gt] * n, 1) + 0.01 * rn(B, n, R, R)
        return {
            "csmri_admm": (cstate(3), cs, cs, (sig, mu)),
            "csmri_hqs": (cstate(2), cs, cs, (sig, mu)),
            "csmri_pg": (cstate(1), cs, cs, (sig, tau)),
            "csmri_apg": (cstate(2), cs, cs, (sig, tau, beta)),
            "csmri_redadmm": (cstate(3), cs, cs, (sig, mu, lam)),
            "pr_iadmm": (pstate(3), pr, pr, (sig, mu, tau)),
            "pr_pg": (pstate(1), pr, pr, (sig, tau)),
            "spi_admm": (torch.cat([spi[0]] * 3, 1) + 0.01 * rn(B, 3, H, H), spi, spi, (sig, mu)),
            "ct_iadmm": (cts(3), ct, ct[1:], (sig, mu, tau)),
            "ct_pg": (cts(1), ct, ct[1:], (sig, tau)),
        }, (cstate(2), cs, sig, rn(T, B, 1, H, H))

    for tag, mode, guard, shapes in (("m0", 0, None, ((2, 64), (1, 256))), ("m1", 1, None, ((2, 64), (1, 256))),
                                     ("m1g2", 1, 2, ((2, 64),))):
        ctx = ops.Context(dev)
        ctx.load_unet(params)
        ctx.set_option("conv_mode", mode)
        if guard is not None:
            ctx.set_option("range_guard", guard)
        for B, H in shapes:
            fams, amp = families(ctx, B, H)
            for name, (state, aux, baux, hy) in fams.items():
                gout = rn(*state.shape)
                for it, itag in ((None, f"T{T}"), (ITER, f"iter{ITER}")):
                    k = f"{tag}/{B}x{H}/{name}/{itag}/"
                    keep(k + "fwd_state", getattr(ops, name)(ctx, state, *aux, *hy, it))
                    o, saved, ticket = getattr(ops, name + "_train")(ctx, state, *aux, *hy, it)
                    keep(k + "train_state", o)
                    keep(k + "train_saved", saved)
                    keep(k + "train_ticket_nonzero", bool(ticket))
                    for btag, tk in (("bwd_ticket", ticket), ("bwd_recompute", 0)):
                        g = getattr(ops, name + "_backward")(ctx, *baux, *hy, saved, gout, it, tk)
                        for i, gi in enumerate(g):
                            keep(k + f"{btag}_g{i}", gi)
                    print(k, "ticket", ticket, flush=True)
            v, cs, sig, probe = amp
            for it, itag in ((None, f"T{T}"), (ITER, f"iter{ITER}")):
                keep(f"{tag}/{B}x{H}/csmri_amp/{itag}/fwd_state", ops.csmri_amp(ctx, v, *cs, sig, probe, it))
        ctx.status()
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print(f"wrote {len(out)} arrays, {sum(v.size for v in out.values())} elements, to {out_path}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
