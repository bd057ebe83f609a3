"""Writes tests/golden/policy_actor_grad.npz from the EXECUTED reference actor's autograd in train mode: the reference's own
ResNetActor_HQS(5, 5) (tfpnp/policy/network.py, SynchronizedBatchNorm2d on one device) in float64 with synthetic weights, one
`.train()` forward on one seeded observation, loss = sum(gp * probs) + sum(gd * det), loss.backward().  Build machine only: it
needs the reference checkout and never runs on a GPU box.

    python tools/make_actor_grad_golden.py

Weights, observation and upstream gradients are those of tests/actor_grad_cases.py for CASE / SHAPE (regenerated from the seeds by
tests/test_actor_grad_host.py).  The file stores data only: per gradient tensor (synth.policy_param_specs order without the running
statistics) its float64 L2 norm and its values at 256 seeded positions (tests/actor_grad_cases.py::sample_positions), and the loss.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import actor_grad_cases as G  # noqa: E402
from tests import actor_train_cases as T  # noqa: E402
from tfpnp_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "policy_actor_grad.npz")
CASE, SHAPE = G.GOLDEN_CASE, G.GOLDEN_SHAPE


def main():
    assert ref_shim.available(), "reference not mounted"
    ref_shim.install()
    torch.set_num_threads(8)
    from tfpnp.policy.network import ResNetActor_HQS
    actor = ResNetActor_HQS(5, 5)
    params = T.params(CASE)
    sd = actor.state_dict()
    assert [k for k, v in sd.items() if v.dtype == torch.float32] == [k for k, _ in synth.policy_param_specs(*CASE)]
    with torch.no_grad():
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(v))
    actor.double().train()
    ob = torch.from_numpy(T.observation(CASE, SHAPE)).double()
    gp, gd = (torch.from_numpy(a).double() for a in G.upstream(CASE, SHAPE))
    got = {}
    actor.fc_softmax.register_forward_hook(lambda m, i, o: got.__setitem__("probs", o))
    actor.fc_deterministic.register_forward_hook(lambda m, i, o: got.__setitem__("det", o))
    actor(ob, torch.zeros(SHAPE[0], dtype=torch.long), True, None)   # the reference's own forward, in train mode
    loss = (gp * got["probs"]).sum() + (gd * got["det"]).sum()
    loss.backward()
    named = dict(actor.named_parameters())
    keys = [k for k, _, _ in G.tensors(CASE)]
    norms = np.array([float(named[k].grad.norm()) for k in keys], np.float64)
    samples = np.stack([named[k].grad.reshape(-1)[torch.from_numpy(G.sample_positions(n))].numpy() for k, _, n in G.tensors(CASE)])
    np.savez_compressed(OUT, case=np.array(CASE, np.int64), shape=np.array(SHAPE, np.int64), loss=np.float64(loss.detach()), norms=norms,
                        samples=samples.astype(np.float64))
    print(f"loss {float(loss.detach()):.6f}; {len(keys)} tensors; wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KB)")


if __name__ == "__main__":
    main()
