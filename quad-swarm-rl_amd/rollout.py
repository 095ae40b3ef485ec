"""A rollout segment - T control steps of [policy encoder -> action head -> environment step] - captured once into a HIP graph.

The stepper's launch (`qs_step`: one hipModuleLaunchKernel, its per-environment step counters live in device memory) and the fused
encoder's launches are stream-ordered and allocation-free, so the whole closed loop can be recorded on a capturing stream and
replayed with one host call per segment: no Python, no per-launch host cost (about 4 us per launch on this platform) inside the
segment.  This is the device-resident counterpart of a Sample Factory rollout worker's inner loop (the reference steps its
environments from `swarm_rl/train.py` through SF's sampler); it needs no part of SF.

    seg = GraphedRollout(env, encoder, head, steps=32)
    out = seg.run()          # dict of device tensors: obs[T, A, D], actions[T, A, 4], means[T, A, 4], rewards[T, A], dones[T, A], last_obs[A, D]
                             # (record_neighbor_ids=True: + neighbor_ids[T, A, K], the drone behind each neighbour slot of obs[t])

With a critic the segment also finishes the batch for a PPO learner, still inside the one graph:

    critic = FusedQuadEncoder(critic_module, precision="fp32"); critic.set_head(value.weight, value.bias)      # a 1-row head
    seg = GraphedRollout(env, encoder, head, steps=128, critic=critic, targets=dict(gamma=0.99, gae_lambda=1.0, reward_scale=1.0, reward_clip=10.0))
    out = seg.run()          # ... + values[T + 1, A], logp[T, A], advantages[T, A], returns[T, A]
"""
from . import native


class GaussianActionHead:
    """mean = Linear(in_features, 4)(features) - in_features = the encoder's out_dim: 512, 256 for Sim2Real, rnn_size for its narrow widths -, action = mean + exp(log_std) * N(0, 1)  (SF's continuous action parameterisation with a
    state-independent std, `--adaptive_stddev=False` in the reference's runs); `sample=False` returns the mean."""

    def __init__(self, in_features=512, device=0, seed=0, sample=True):
        import torch
        g = torch.Generator().manual_seed(seed)
        dev = torch.device("cuda", device)
        self.weight = (torch.randn((4, in_features), generator=g) * (1.0 / in_features ** 0.5)).to(dev)
        self.bias = torch.zeros(4, device=dev)
        self.log_std = torch.full((4,), -0.5, device=dev)
        self.sample = sample
        self.seed = seed

    def __call__(self, features):
        import torch
        return self.from_mean(torch.addmm(self.bias, features, self.weight.t()))

    def from_mean(self, mean):
        """action from the Linear's output; GraphedRollout gets that from the encoder's fused epilogue (FusedQuadEncoder.forward_head)"""
        import torch
        if not self.sample:
            return mean
        return mean + torch.exp(self.log_std) * torch.randn_like(mean)


class GraphedRollout:
    TARGET_KEYS = ("gamma", "gae_lambda", "reward_scale", "reward_clip")

    def __init__(self, env, encoder, head, steps, graph=True, critic=None, targets=None, critic_chunk=65536, record_neighbor_ids=False):
        """env: QuadSwarmVecEnv (float32), encoder: policy.FusedQuadEncoder, head: features[A, encoder.out_dim] -> actions[A, 4].
        Construction runs ONE control step eagerly (library warm-up outside the capture) before recording.

        With the library's GaussianActionHead the segment has no glue launches at all: the encoder's epilogue evaluates the head AND
        samples the action into actions[t] (qs_enc_params.sample_*); the step writes its observation rows straight into obs[t + 1]
        (qs_set_obs_target); its rewards / done flags are copied into rewards[t] / dones[t] by the first kernel of the NEXT step's forward pass
        (qs_enc_params.traj_*; round 5 - a launch of its own, qs_rollout_post, until round 4 and still for the segment's last step).
        2 (attention: 3) dependent graph nodes per control step, and no observation copy.  Measured on C2, us per control step
        (profiles/r05h_bench_rollout.txt): mean_embed 31.5, attention 82.5; with a copy launch of its own per step 33.0 (round 4); the copy on a
        second stream as a parallel graph branch 46.3 - a fork / join costs more than the launch it hides; rewards / done redirected inside the
        step kernel 31.8, but + 0.08 us on every step of every user of the headline kernel - not taken.
        `means[t]` keeps the action head's output of every step - the mean of the Gaussian the action was drawn from - so that a learner has the
        behaviour policy's log-probabilities without a second forward pass (tools/ppo_c5.py).

        critic: a FusedQuadEncoder (not `encoder`) with a 1-row head (set_head(value_weight, value_bias)): the segment also fills
        values[T + 1, A] - batched forward_head launches over the recorded observations in slices of `critic_chunk` rows plus one over last_obs,
        all BEHIND the last step (a dependent launch or a forked branch per step costs more than it hides, see above, and large batches run on
        the encoder's throughput kernels).  targets = dict(gamma, gae_lambda, reward_scale, reward_clip), needs `critic`: one more launch
        (qs_rollout_targets) turns rewards / dones / values into GAE advantages and returns, and means / actions / the head's log_std into the
        behaviour policy's log-probabilities (a sampling head only) - Learner.advantages / gaussian_logp of tools/ppo_c5.py on the device.
        The critic's weights follow its module through critic.refresh(); for an `attention` critic recapture() afterwards, as for the actor.

        record_neighbor_ids: the segment also records neighbor_ids[T, A, K] (int32) - the drone behind each neighbour slot of the rows the policy
        read at step t (include/quadswarm_neighbors.h: -1 where no drone matches) - with one more launch per control step, in front of the
        step while the state is still that of the rows.  Off, the segment has the launches it had."""
        import torch
        if targets is not None:
            if critic is None:
                raise ValueError("targets needs a critic: advantages and returns are built on its values")
            if sorted(targets) != sorted(self.TARGET_KEYS):
                raise ValueError(f"targets: a dict with exactly the keys {self.TARGET_KEYS}")
        if critic is not None and (critic is encoder or critic_chunk < 1):
            raise ValueError("critic: an encoder object of its own (its head is the value layer), critic_chunk >= 1")
        if not torch.cuda.is_available():
            raise native.QsError("GraphedRollout needs a GPU")
        if env.stepper.real_size != 4:
            raise ValueError("the policy path is float32")
        self.env, self.encoder, self.head, self.steps = env, encoder, head, steps
        self.critic, self.targets, self.critic_chunk = critic, dict(targets) if targets is not None else None, int(critic_chunk)
        if critic is not None and (getattr(critic, "_head", None) is None or critic._head[0].shape[0] != 1):
            raise ValueError("critic: call set_head(value_weight [1, features], value_bias [1]) on it first")
        st = env.stepper
        self._obs, self._rew, self._done = st.tensor("obs"), st.tensor("reward"), st.tensor("done")
        A, D = self._obs.shape
        dev = self._obs.device
        new = torch.empty if critic is None else torch.zeros   # (the warm-up's critic pass and target launch read every slot: defined contents)
        self.obs = new((steps, A, D), device=dev)
        self.actions = new((steps, A, 4), device=dev)
        self.rewards = new((steps, A), device=dev)
        self.dones = new((steps, A), device=dev, dtype=torch.uint8)
        self.neighbor_ids = None
        if record_neighbor_ids:
            if int(env.cfg.num_neighbors) < 1:
                raise ValueError("record_neighbor_ids: the environment's rows have no neighbour slots")
            self.neighbor_ids = torch.full((steps, A, int(env.cfg.num_neighbors)), -1, device=dev, dtype=torch.int32)
        if critic is not None:
            self.values = torch.zeros((steps + 1, A), device=dev)
        if targets is not None:
            self.advantages, self.returns = torch.zeros((steps, A), device=dev), torch.zeros((steps, A), device=dev)
        self._fused_head = hasattr(head, "from_mean") and hasattr(head, "weight") and hasattr(encoder, "set_head")
        self._glue = False
        if self._fused_head:   # the Linear runs in the encoder's epilogue: the [A, out_dim] features are never written
            encoder.set_head(head.weight, head.bias)
            self.means = new((steps, A, 4), device=dev)   # the action head's output per step
            # ... and with the library's head so do sampling and the trajectory writes (no copy / sampling kernels between the steps)
            self._glue = isinstance(head, GaussianActionHead) and self.dones.dtype == torch.uint8 and self._done.dtype == torch.uint8
            # (the device-side replay wrapper restores observations into the library's buffer and reads its done flags: a handle with
            # replay enabled keeps its outputs there, and the segment copies them - the two glue launches of qs_rollout_pre / _post)
            self._in_place = self._glue and not getattr(st, "replay_on", False)
            if self._glue:
                self._counter = torch.zeros(1, device=dev, dtype=torch.int32)
                self._scratch_counter = torch.zeros(1, device=dev, dtype=torch.int32)   # (qs_rollout_post's own counter: unused here)
                self._seed = int(getattr(head, "seed", 0)) & 0xffffffffffffffff
        else:
            self._feat = torch.empty((A, encoder.out_dim), device=dev)
        # log-probabilities: of SAMPLED actions under the recorded means (a deterministic head has no density to report)
        self._want_logp = targets is not None and self._fused_head and bool(getattr(head, "sample", True)) and hasattr(head, "log_std")
        if self._want_logp:
            self.logp = torch.zeros((steps, A), device=dev)
        self.graph = None
        try:
            if graph:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    self._segment(1)     # one step, eagerly: library warm-up outside the capture (+ the critic at the capture's batch sizes)
                torch.cuda.current_stream(dev).wait_stream(side)
                self.recapture()
        finally:
            self._restore_targets()

    def recapture(self):
        """Record the segment again.  Needed when something that travels in LAUNCH ARGUMENTS changed - the attention encoder's score bias after
        FusedQuadEncoder.refresh(), the head's sampling switch; weights, log-std, reward coefficients live in device memory and are picked up
        by replays of the old graph.  Capturing runs nothing: the environments stay where they are."""
        import torch
        dev = self._obs.device
        torch.cuda.synchronize(dev)
        try:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._segment(self.steps)
        finally:
            self._restore_targets()

    def warmup(self):
        """one control step outside any capture (what the constructor does before it records a graph)"""
        try:
            self._segment(1)
        finally:
            self._restore_targets()

    def _restore_targets(self):
        """the stepper's output redirections are host-side launch state: an env.step() outside the segment writes the library's buffers"""
        if self._glue and self._in_place:
            self.env.stepper.set_obs_target(None)

    def _segment(self, n):
        """n control steps from the environments' current state, then - with a critic - the values / targets of the WHOLE buffer (in the one-step
        warm-up too: the attention critic's scratch grows on first use, so it has to see the capture's batch sizes outside the capture)"""
        self._steps(n)
        if self.critic is not None:
            self._finish()

    def _finish(self):
        """values[T + 1, A] from the critic over the recorded observations (+ last_obs), then qs_rollout_targets"""
        from . import policy
        TA, D = self.steps * self._obs.shape[0], self._obs.shape[1]
        flat, vals = self.obs.reshape(TA, D), self.values.reshape(-1, 1)
        for s0 in range(0, TA, self.critic_chunk):
            s1 = min(TA, s0 + self.critic_chunk)
            self.critic.forward_head(flat[s0:s1], head_out=vals[s0:s1])
        self.critic.forward_head(self._obs, head_out=vals[TA:])
        if self.targets is not None:
            lp = dict(means=self.means, actions=self.actions, log_std=self.head.log_std, logp=self.logp) if self._want_logp else {}
            policy.rollout_targets(self.rewards, self.dones, self.values, advantages=self.advantages, returns=self.returns, **self.targets, **lp)

    def _steps(self, n):
        """n control steps from the environments' current state"""
        if self._glue and not self._in_place:
            for t in range(n):
                self._step_copying(t)
            return
        if self._glue:
            import ctypes as C
            import torch
            from . import policy
            st, last, A = self.env.stepper, n - 1, self._obs.shape[0]
            main = self._torch_stream()
            self.obs[0].copy_(self._obs)      # the one observation copy of the segment: the rows the environments are in
            for t in range(n):
                # the reward / done flags of step t - 1 ride on this forward pass's first kernel (qs_enc_params.traj_*): two dependent launches per
                # control step (three with `attention`) instead of three (four); only the LAST step of the segment needs a copy launch of its own
                traj = (self._rew, self.rewards[t - 1], self._done, self.dones[t - 1]) if t > 0 else None
                if self.head.sample:
                    self.encoder.forward_head(self.obs[t], head_out=self.means[t], sample=(self.head.log_std, self.actions[t], self._counter, t, self._seed), traj=traj)
                else:   # deterministic policy: the head's output IS the action
                    self.encoder.forward_head(self.obs[t], head_out=self.actions[t], traj=traj)
                # step t: observation rows -> obs[t + 1] (the last step: the library's buffer, where the next segment starts)
                if self.neighbor_ids is not None:   # the state is still the one the rows obs[t] were written from
                    st.neighbor_ids(obs=self.obs[t], out=self.neighbor_ids[t], stream=main)
                st.set_obs_target(self.obs[t + 1].data_ptr() if t < last else None)
                st.step(self.actions[t].data_ptr(), stream=main)
            rc = policy.lib().qs_rollout_post(C.c_void_p(self._rew.data_ptr()), C.c_void_p(self.rewards[last].data_ptr()), C.c_void_p(self._done.data_ptr()),
                                              C.c_void_p(self.dones[last].data_ptr()), A, C.c_void_p(self._scratch_counter.data_ptr()), C.c_void_p(main.cuda_stream))
            if rc != 0:
                raise native.QsError(f"qs_rollout_post failed ({rc})")
            self._counter.add_(n)             # the next replay draws fresh noise
            return
        for t in range(n):
            self._step(t)

    def _torch_stream(self):
        import torch
        return torch.cuda.current_stream(self._obs.device)

    def _step_copying(self, t):
        """the segment step of a handle whose outputs stay in the library's buffers: sampling + observation copy in one launch before
        the step, reward / done copies + counter in one launch behind it"""
        import ctypes as C
        from . import policy
        L = policy.lib()
        stream = C.c_void_p(self._torch_stream().cuda_stream)
        A = self._obs.shape[0]
        self.encoder.forward_head(self._obs, head_out=self.means[t])
        log_std = C.c_void_p(self.head.log_std.data_ptr()) if self.head.sample else None
        rc = L.qs_rollout_pre(C.c_void_p(self._obs.data_ptr()), C.c_void_p(self.obs[t].data_ptr()), self._obs.numel(), C.c_void_p(self.means[t].data_ptr()), log_std,
                              C.c_void_p(self.actions[t].data_ptr()), A, C.c_uint64(self._seed), C.c_void_p(self._counter.data_ptr()), stream)
        if rc != 0:
            raise native.QsError(f"qs_rollout_pre failed ({rc})")
        if self.neighbor_ids is not None:
            self.env.stepper.neighbor_ids(out=self.neighbor_ids[t], stream=self._torch_stream())
        self.env.stepper.step(self.actions[t].data_ptr(), stream=self._torch_stream())
        rc = L.qs_rollout_post(C.c_void_p(self._rew.data_ptr()), C.c_void_p(self.rewards[t].data_ptr()), C.c_void_p(self._done.data_ptr()),
                               C.c_void_p(self.dones[t].data_ptr()), A, C.c_void_p(self._counter.data_ptr()), stream)
        if rc != 0:
            raise native.QsError(f"qs_rollout_post failed ({rc})")

    def _step(self, t):
        self.obs[t].copy_(self._obs)
        if self._fused_head:
            self.encoder.forward_head(self._obs, head_out=self.means[t])
            self.actions[t].copy_(self.head.from_mean(self.means[t]))
        else:
            self.encoder(self._obs, out=self._feat)
            self.actions[t].copy_(self.head(self._feat))
        if self.neighbor_ids is not None:
            self.env.stepper.neighbor_ids(out=self.neighbor_ids[t], stream=self._torch_stream())
        self.env.stepper.step(self.actions[t].data_ptr(), stream=self._torch_stream())
        self.rewards[t].copy_(self._rew)
        self.dones[t].copy_(self._done)

    def run(self):
        """One segment of `steps` control steps from the environments' current state (stream-ordered, asynchronous).  The returned
        tensors are the segment's buffers: the next run() overwrites them."""
        if self.graph is not None:
            self.graph.replay()
        else:
            try:
                self._segment(self.steps)
            finally:
                self._restore_targets()
        out = {"obs": self.obs, "actions": self.actions, "rewards": self.rewards, "dones": self.dones, "last_obs": self._obs}
        if self._fused_head:
            out["means"] = self.means if getattr(self.head, "sample", True) else self.actions
        if self.neighbor_ids is not None:
            out["neighbor_ids"] = self.neighbor_ids
        if self.critic is not None:
            out["values"] = self.values
        if self.targets is not None:
            out["advantages"], out["returns"] = self.advantages, self.returns
            if self._want_logp:
                out["logp"] = self.logp
        return out
