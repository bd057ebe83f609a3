"""MDDPGTrainer -- tfpnp/trainer/mddpg/trainer.py:20-283 on the native parts of this package: same class name, same constructor
arguments, same methods (`train`, `_update_policy`, `_update`, `run_policy`, `save_experience`, `save_model`, `load_model`) with
the reference's behaviour.

What runs where, per `_update` (trainer.py:158-214):
  actor          native ResNetActor_*: the kept train-mode forward, its parameter gradient, clip + Adam in place
                 (actor_step.py::actor_update, :171 and :201-204)
  policy_loss    ONE launch, torch.ops.pnpx.mddpg_policy_loss (csrc/mddpg_loss.hip): lines 174 and 179-197 and the gradients
                 of the loss with respect to p_stop, V_next and the reward.  From there policy_loss.backward() reaches the
                 deterministic actions along the native VJPs: critic_value's backward (the critic's input gradient), the
                 differentiable get_eval_ob, the solver VJP and PSNR of PnPEnv.forward, and action_mapping
  critic         native ResNet_wobn and its target: value_loss, its gradient, clip + Adam in place and the soft update
                 (critic_step.py::critic_update, :198, :206-212), fed the Q_target the loss launch already wrote, so the target
                 critic is evaluated once per update
  replay memory  device-resident (utils/rpm.py): `save_experience` is one store_batch, `_update_policy` samples whole batches

INITIAL CRITIC.  The native ResNet_wobn has no random initialiser of its own (the reference draws torch's default initialisation).
The critic starts from `opt.critic_state_dict` when the options carry one (a state dict under the reference's key names, e.g. that of
a freshly constructed reference critic), else from synth.make_critic_params(policy.in_dim, seed = opt.seed or 0): synthetic
He-scaled weights, THE SAME ON EVERY RUN unless opt.seed changes.  The logger is minimal (one line per episode to stdout and <log_dir>/log.txt); tensorboardX is optional
and only imported with enable_tensorboard=True.

Out of scope: DataParallel is never built -- multi-GPU training and SyncBN statistics across devices --, Adam's moments are
not saved (the reference's save_model does not save them either), and `_update` is not capturable into a graph (each
optimiser step ends with a small read-back)."""
import os
import time

import torch

from ... import synth
from ... import torch_ops as T
from ...data.batch import Batch
from ...utils.misc import hard_update
from ...utils.rpm import ReplayMemory
from .actor_step import actor_update
from .critic import ResNet_wobn
from .critic_step import critic_update


class Logger:
    """The part of tfpnp/utils/log.py the trainer uses: log(message, color=None) to stdout and <log_dir>/log.txt."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, 'log.txt')

    def log(self, message, color=None):
        print(message)
        with open(self.path, 'a') as f:
            f.write(message + '\n')


class MDDPGTrainer:
    def __init__(self, opt, env, policy, lr_scheduler, device, log_dir, evaluator=None, enable_tensorboard=False, logger=None):
        self.opt = opt
        self.env = env
        self.actor = policy
        self.device = torch.device(device)
        params = getattr(opt, 'critic_state_dict', None)           # the critic's initial weights, under the reference's key names
        if params is None:
            params = synth.make_critic_params(policy.in_dim, getattr(opt, 'seed', None) or 0)
        self.critic = ResNet_wobn(policy.in_dim, 18, 1, state_dict=params)
        self.critic_target = ResNet_wobn(policy.in_dim, 18, 1, state_dict=params)
        self.lr_scheduler = lr_scheduler
        self.evaluator = evaluator
        self.writer = None
        if enable_tensorboard:
            try:
                from tensorboardX.writer import SummaryWriter
            except ImportError as e:
                raise ImportError("MDDPGTrainer(enable_tensorboard=True) needs the tensorboardX package, which is not "
                                  "installed; install it or pass enable_tensorboard=False") from e
            self.writer = SummaryWriter(os.path.join(log_dir, 'tensorboard'))
        self.logger = Logger(log_dir) if logger is None else logger
        self.buffer = ReplayMemory(opt.rmsize * opt.max_episode_step)                  # trainer.py:46
        if self.device.type == 'cuda':
            self.critic.context(self.device)
            hard_update(self.critic_target, self.critic)                               # :53
        # else: a CPU device serves host-logic tests on stubs only (train() with a replaced _update; the native networks
        # have no CPU path, so _update itself raises there).  hard_update needs a device; the two critics were built from the
        # same state dict above, so the target equals the critic without it.
        self.start_step = 1

    # ------------------------------------------------------------------ the loop (behaviour of trainer.py:59-125)
    def _start_episode(self):
        """-> (observation of a fresh batch, the recurrent state of all its rows: a dummy, as in the reference)"""
        ob = self.env.reset()
        return ob, self.actor.init_state(ob.shape[0]).to(self.device)

    def _finish_episode(self, episode, step, best_psnr, started):
        """What follows the last step of an episode: past the warm-up, validation every `validate_interval` episodes (keeping the
        best checkpoint) and `episode_train_times` updates; always one log line.  -> the best validation PSNR so far."""
        opt = self.opt
        training = step > opt.warmup
        if training and self.evaluator is not None and (episode + 1) % opt.validate_interval == 0:
            psnr = self.evaluator.eval(self.actor, step)
            if psnr > best_psnr:
                best_psnr = psnr
                for tag in ('best_{:.2f}'.format(psnr), 'best'):
                    self.save_model(opt.output, tag)
            self.save_model(opt.output)
        rollout_seconds = time.time() - started
        update_started = time.time()
        shown = {'Q': 0, 'dist_entropy': 0, 'critic_loss': 0}
        if training:
            shown, scalars = self._update_policy(opt.episode_train_times, opt.env_batch, step=step)
            if self.writer is not None:
                for name, value in scalars.items():
                    self.writer.add_scalar(f'train/{name}', value, step)
        # the reference's log line, field for field
        self.logger.log('#{}: Steps: {} - RPM[{}/{}] | interval_time: {:.2f} | train_time: {:.2f} | {}'.format(
            episode, step, self.buffer.size(), self.buffer.capacity, rollout_seconds, time.time() - update_started,
            ' | '.join(f'{k}: {v:.2f}' for k, v in shown.items())))
        return best_psnr

    def train(self):
        opt = self.opt
        ob, hidden_all = self._start_episode()
        hidden = hidden_all
        episode, steps_taken, best_psnr, started = 0, 0, 0, time.time()
        for step in range(self.start_step, opt.train_steps + 1):
            action, hidden = self.run_policy(self.env.get_policy_ob(ob), hidden)
            _, ob_live, _, all_stopped, _ = self.env.step(action)
            steps_taken += 1
            self.save_experience(ob, hidden)          # the state BEFORE the step, all of its rows: the update re-runs the step
            ob, hidden = ob_live, hidden_all[self.env.idx_left, ...]

            if all_stopped or steps_taken == opt.max_episode_step:
                best_psnr = self._finish_episode(episode, step, best_psnr, started)
                ob, hidden_all = self._start_episode()
                hidden = hidden_all
                episode, steps_taken, started = episode + 1, 0, time.time()

            if step % opt.save_freq == 0 or step == opt.train_steps:
                if self.evaluator is not None:        # (the reference dereferences its optional evaluator here)
                    self.evaluator.eval(self.actor, step)
                self.logger.log('Saving model at Step_{:07d}...'.format(step))
                self.save_model(opt.output, step)

    # ------------------------------------------------------------------ updates after an episode (trainer.py:127-156)
    _DIAGNOSTICS = ('Q', 'critic_loss', 'dist_entropy', 'actor_norm', 'critic_norm')      # the order _update returns them in

    def _update_policy(self, episode_train_times, env_batch, step):
        """`episode_train_times` updates on freshly sampled batches at the learning rates of `step`.
        -> (the means the log line shows, the scalars a tensorboard writer gets): the reference's two dicts."""
        self.actor.train()
        lr = self.lr_scheduler(step)
        total = None
        for _ in range(episode_train_times):
            batch = self.buffer.sample(env_batch)                  # the batch convert2batch(sample_batch(env_batch)) builds
            out = torch.stack([x.reshape(()).float() for x in self._update(samples=batch, lr=lr)])
            total = out if total is None else total + out
        mean = dict(zip(self._DIAGNOSTICS, (total / episode_train_times).tolist()))       # the one host read of the call
        scalars = {'critic_lr': lr['critic'], 'actor_lr': lr['actor']}
        scalars.update((k, mean[k]) for k in ('Q', 'dist_entropy', 'critic_loss', 'actor_norm', 'critic_norm'))
        shown = {'Q': mean['Q'], 'dist_entropy': mean['dist_entropy'], 'closs': mean['critic_loss'], 'anorm': mean['actor_norm'],
                 'cnorm': mean['critic_norm']}
        return shown, scalars

    # ------------------------------------------------------------------ trainer.py:158-214
    def _update(self, samples, lr, idx_stop=None):
        """One update on `samples` (a list of row Batches, or the Batch they stack to); lr: {'actor': ., 'critic': .};
        idx_stop [B] int64: teacher-forced stop decisions (None: sampled, as the reference does).
        -> (-policy_loss, value_loss, mean entropy, actor_norm, critic_norm): 0-dim device tensors, nothing is read back here."""
        opt, env = self.opt, self.env
        ob = samples if isinstance(samples, Batch) else Batch.stack(samples)
        ob = ob.to(self.device)
        policy_ob = env.get_policy_ob(ob)
        eval_ob = env.get_eval_ob(ob)
        kept = {}

        def loss_fn(action, action_log_prob, dist_entropy, p_stop):
            # log-probability and entropy are taken again inside the loss launch, from p_stop: the head's copies are not used
            ob2, reward = env.forward(ob, action)                                          # :173
            eval_ob2 = env.get_eval_ob(ob2)                                                # :177, differentiable
            with torch.no_grad():
                V_cur = self.critic(eval_ob)                                               # :180 (detached by :186)
                V_next_target = self.critic_target(eval_ob2.detach())                      # :182
            V_next = self.critic(eval_ob2)                                                 # :190
            scalars, Q_target, _, _, _, _, _ = T.call(
                "mddpg_policy_loss", p_stop, action['idx_stop'], V_cur, V_next_target, V_next, reward,
                float(opt.discount), float(opt.loop_penalty), float(opt.lambda_e))         # :174, :183-197
            kept.update(Q_target=Q_target, mean_entropy=scalars[1].detach())
            return scalars[0]

        # ORDER.  actor_update differentiates policy_loss completely -- the critic's input gradient at the weights V_next was
        # evaluated with, the solver VJP, the actor's parameter gradient -- before its adam_step_ moves the actor, and the critic
        # moves only afterwards: the actor steps before the critic (:201-209), and neither network changes under a backward
        # pass that still reads it.  The target follows last (:212, inside critic_update).
        a = actor_update(self.actor, policy_ob, loss_fn, lr['actor'], max_norm=50, idx_stop=idx_stop, pass_probs=True)
        c = critic_update(self.critic, self.critic_target, eval_ob, None, None, None, opt.discount, opt.tau, lr['critic'],
                          max_norm=50, q_target=kept['Q_target'])
        return -a['policy_loss'], c['value_loss'], kept['mean_entropy'], a['actor_norm'], c['critic_norm']

    # ------------------------------------------------------------------ trainer.py:216-241
    def run_policy(self, ob, hidden=None):
        self.actor.eval()
        with torch.no_grad():
            action, _, _, hidden = self.actor(ob, None, True, hidden)
        self.actor.train()
        return action, hidden

    def save_experience(self, ob, hidden):
        self.buffer.store_batch(ob, hidden)           # all rows in one launch; nothing visits the host

    # ------------------------------------------------------------------ trainer.py:243-272
    def save_model(self, path, step=None):
        """ckpt/actor[_postfix].pkl and ckpt/critic[_postfix].pkl: state dicts under the reference's key names (CPU tensors)."""
        path = os.path.join(path, 'ckpt')
        os.makedirs(path, exist_ok=True)
        postfix = '' if step is None else '_' + (step if isinstance(step, str) else '{:07d}'.format(step))
        for name, net in (('actor', self.actor), ('critic', self.critic)):
            state = net.state_dict()
            torch.save(type(state)((k, v.cpu()) for k, v in state.items()), '{}/{}{}.pkl'.format(path, name, postfix))

    def load_model(self, path, step=None):
        """`path` is the ckpt directory itself, as in the reference; the target critic is not touched (nor is it there)."""
        postfix = ''
        if step is not None:
            self.start_step = step
            postfix = '_{:07d}'.format(step)
        self.actor.load_state_dict(torch.load('{}/actor{}.pkl'.format(path, postfix)))
        self.critic.load_state_dict(torch.load('{}/critic{}.pkl'.format(path, postfix)))
