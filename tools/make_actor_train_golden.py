"""Writes tests/golden/policy_actor_train.npz from the EXECUTED reference actor in train mode: the reference's own
ResNetActor_HQS(5, 5) (tfpnp/policy/network.py, SynchronizedBatchNorm2d on one device) with synthetic weights, two
`.train()` forwards on one seeded observation.  Build machine only: it needs the reference checkout and never runs on a GPU
box.

    python tools/make_actor_train_golden.py

Weights are synth.make_policy_params(7, 10, False, WEIGHT_SEED) and the observation RandomState(OB_SEED).uniform(0, 1) of
shape SHAPE; the file stores outputs and running statistics only (tests/test_actor_train_host.py regenerates the inputs
from the seeds): probs, det, log-probability and entropy for IDX_STOP, and every running statistic after each forward.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tfpnp_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "policy_actor_train.npz")
CASE = (7, 10, False)
WEIGHT_SEED, OB_SEED = 3, 11
SHAPE = (3, 7, 32, 96)
IDX_STOP = (0, 1, 1)


def main():
    assert ref_shim.available(), "reference not mounted"
    ref_shim.install()
    torch.set_num_threads(8)
    from tfpnp.policy.network import ResNetActor_HQS
    actor = ResNetActor_HQS(5, 5)
    params = synth.make_policy_params(*CASE, seed=WEIGHT_SEED)
    sd = actor.state_dict()
    assert [k for k, v in sd.items() if v.dtype == torch.float32] == [k for k, _ in synth.policy_param_specs(*CASE)]
    with torch.no_grad():
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(v))
    actor.train()
    ob = torch.from_numpy(np.random.RandomState(OB_SEED).uniform(0, 1, SHAPE).astype(np.float32))
    idx_stop = torch.tensor(IDX_STOP)
    res = {"weight_seed": np.int64(WEIGHT_SEED), "ob_seed": np.int64(OB_SEED), "shape": np.array(SHAPE),
           "idx_stop": np.array(IDX_STOP)}
    stat_keys = [k for k, _ in synth.policy_param_specs(*CASE) if k.endswith("running_mean") or k.endswith("running_var")]
    got = {}
    actor.fc_softmax.register_forward_hook(lambda m, i, o: got.__setitem__("probs", o.detach()))
    actor.fc_deterministic.register_forward_hook(lambda m, i, o: got.__setitem__("det", o.detach()))
    for it in (1, 2):
        with torch.no_grad():
            _, logp, entropy, _ = actor(ob, idx_stop, True, None)   # the reference's own forward, in train mode
        probs = got["probs"]
        res[f"probs{it}"] = probs.numpy()
        res[f"det{it}"] = got["det"].numpy()
        res[f"logp{it}"] = logp.numpy()
        res[f"entropy{it}"] = entropy.numpy()
        now = actor.state_dict()
        res[f"running{it}"] = np.concatenate([now[k].numpy().reshape(-1) for k in stat_keys])
        print(f"forward {it}: probs {probs[0].tolist()}  |running| {np.abs(res[f'running{it}']).max():.4f}", flush=True)
    np.savez_compressed(OUT, **res)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KB)")


if __name__ == "__main__":
    main()
