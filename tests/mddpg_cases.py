"""Yardstick of the MDDPG policy-loss tests: a restatement of tfpnp/trainer/mddpg/trainer.py:174-197 in torch, evaluated in the
dtype of its inputs, so that torch's own autograd gives the reference gradients.  log-probability and entropy are those of
ResNetActorBase.head / torch's Categorical (tfpnp/policy/network.py:149-161): clamp_min with float32's eps -- in float64 too --
and xlogy.  No GPU needed to import, no reference import (the reference trainer imports tensorboardX, which is not installed).

THE BAR (tests/test_gpu_mddpg.py).  For every output, elementwise:
    |kernel - fp64| <= 4 * |fp32 - fp64| + 2 * ulp32(largest term)
where fp64 / fp32 are this restatement on the same float32 inputs, evaluated by torch on the CPU in float64 / float32.  The
factor 4 allows for a logf with other roundings than the host's and another order of the same fp32 operations; the second summand
is the rounding of a result whose summands cancel (and of an fp32 evaluation that happens to be exact).  `terms` returns the
largest term per output: the largest absolute value among the summands of the last sum that forms it (for the two means: among
the rows' summands).
"""
import torch

EPS32 = float(torch.finfo(torch.float32).eps)
DISCOUNT, LOOP_PENALTY, LAMBDA_E = 0.99, 0.05, 0.2
OUTPUTS = ("policy_loss", "mean_entropy", "q_target", "log_prob", "entropy", "grad_p_stop", "grad_v_next", "grad_reward")


def inputs(B, seed, kind="random"):
    """float32 / int64 CPU tensors: p_stop = softmax of N(0, 2^2) logits, values 5 * N(0, 1), rewards N(0, 1), both idx_stop
    values present whenever B > 1.  kind 'clamp': logits +-20, so the taken probability of every second row is below eps;
    kind 'stopped': every row stops."""
    gen = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=gen)
    logits = 2.0 * n(B, 2)
    idx = torch.randint(0, 2, (B,), generator=gen)
    if B > 1:
        idx[0], idx[1] = 0, 1
    if kind == "clamp":
        logits = torch.tensor([[20.0, -20.0]]).repeat(B, 1)
        logits[::2] = -logits[::2]
        idx = torch.zeros(B, dtype=torch.int64)          # even rows: p0 = softmax(-20, 20)[0] ~ 4e-18 < eps
    if kind == "stopped":
        idx = torch.ones(B, dtype=torch.int64)
    return dict(p_stop=torch.softmax(logits, 1), idx_stop=idx, v_cur=5 * n(B), v_next_target=5 * n(B), v_next=5 * n(B), reward=n(B))


def pieces(p_stop, idx_stop, v_cur, v_next_target, v_next, reward, discount=DISCOUNT, loop_penalty=LOOP_PENALTY, lambda_e=LAMBDA_E):
    """trainer.py:174-197 on [B] vectors, in the dtype of p_stop.  -> dict with policy_loss and everything it is made of."""
    r = reward - loop_penalty                                                             # :174
    g = discount * (1 - idx_stop.to(p_stop.dtype))                                        # :184, :191
    logp = torch.log(p_stop.clamp_min(EPS32)).gather(1, idx_stop.view(-1, 1)).squeeze(1)  # network.py head / Categorical.log_prob
    ent = -torch.special.xlogy(p_stop, p_stop).sum(dim=1)                                 # Categorical.entropy
    with torch.no_grad():
        q_target = g * v_next_target + r                                                  # :182-185
    adv = (q_target - v_cur).clone().detach()                                             # :186
    a2c = logp * adv                                                                      # :187
    ddpg = g * v_next + r                                                                 # :190-192
    policy_loss = -(a2c + ddpg + lambda_e * ent).mean()                                   # :197
    return dict(policy_loss=policy_loss, mean_entropy=ent.mean(), q_target=q_target, log_prob=logp, entropy=ent, adv=adv, g=g, r=r,
                a2c=a2c, ddpg=ddpg)


def restate(case, dtype):
    """The eight OUTPUTS of the restatement on `case` (inputs()) in `dtype` at the module's DISCOUNT, LOOP_PENALTY and LAMBDA_E,
    gradients by torch autograd, as float64 CPU tensors, plus the pieces ('adv', 'g', 'r', 'a2c', 'ddpg')."""
    x = {k: (v.clone() if k == "idx_stop" else v.detach().clone().to(dtype)) for k, v in case.items()}
    leaves = [x[k].requires_grad_() for k in ("p_stop", "v_next", "reward")]
    out = pieces(**x)
    grads = torch.autograd.grad(out["policy_loss"], leaves)
    out.update(grad_p_stop=grads[0], grad_v_next=grads[1], grad_reward=grads[2])
    return {k: v.detach().double() for k, v in out.items()}


def closed_form_grads(case, ref):
    """The gradients as the issue states them, from float64 pieces `ref` (restate(case, float64))."""
    p = case["p_stop"].double()
    idx = case["idx_stop"]
    B = p.shape[0]
    gp = LAMBDA_E * (torch.log(p) + 1) / B
    taken = p.gather(1, idx.view(-1, 1)).squeeze(1)
    a2c = torch.where(taken >= EPS32, -ref["adv"] / (B * taken), torch.zeros_like(taken))
    gp = gp.scatter_add(1, idx.view(-1, 1), a2c.view(-1, 1))
    return dict(grad_p_stop=gp, grad_v_next=-ref["g"] / B, grad_reward=torch.full((B,), -1.0 / B, dtype=torch.float64))


def ulp32(x):
    """Spacing of float32 at |x| (float64 tensor in, float64 tensor out; at least the smallest normal's spacing)."""
    a = x.abs().clamp_min(2.0 ** -126)
    return 2.0 ** (torch.floor(torch.log2(a)) - 23)


def terms(case, ref):
    """Largest term per output (see the module docstring), float64, broadcastable to the output."""
    p = case["p_stop"].double()
    idx = case["idx_stop"]
    B = p.shape[0]
    mx = lambda *a: torch.stack([t.abs() for t in torch.broadcast_tensors(*a)]).amax(0)
    row = mx(ref["a2c"], ref["g"] * case["v_next"].double(), ref["r"], LAMBDA_E * ref["entropy"])
    taken = p.gather(1, idx.view(-1, 1)).squeeze(1)
    ent_part = LAMBDA_E * mx(torch.log(p), torch.ones_like(p)) / B
    a2c = torch.where(taken >= EPS32, (ref["adv"] / (B * taken)).abs(), torch.zeros_like(taken))      # no a2c term under the clamp
    a2c_part = torch.zeros_like(p).scatter(1, idx.view(-1, 1), a2c.view(-1, 1))
    return dict(policy_loss=row.max(), mean_entropy=ref["entropy"].abs().max(),
                q_target=mx(ref["g"] * case["v_next_target"].double(), ref["r"]), log_prob=ref["log_prob"].abs(),
                entropy=torch.special.xlogy(p, p).abs().amax(1), grad_p_stop=mx(ent_part, a2c_part),
                grad_v_next=ref["g"].abs() / B, grad_reward=torch.full((B,), 1.0 / B, dtype=torch.float64))


def bars(case):
    """-> (fp64 outputs, per output the bound of the module docstring)"""
    ref, f32 = restate(case, torch.float64), restate(case, torch.float32)
    t = terms(case, ref)
    return ref, {k: 4.0 * (f32[k] - ref[k]).abs() + 2.0 * ulp32(t[k]) for k in OUTPUTS}


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (got: any float tensor; compared in float64 on the CPU)."""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    return float((err / bound).max())
