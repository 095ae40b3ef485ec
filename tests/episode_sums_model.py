"""The per-episode sums (`episode_sums=1`: qs_buffers.run_sums / ep_sums, include/quadswarm.h:69-73) as a definition: numpy float64, no code
of the package.  What the reference's QuadsRewardShapingWrapper keeps in Python per agent and episode (reward_shaping.py:53, :69-76,
:100-108) - the cumulative reward terms and the list of the actions it was given:

    rows [0, 17)    sum over the episode's steps of each reward term of infos[i]['rewards'] (the order of QS_RI_*)
    rows [17, 21)   sum of the four RAW actions as given to step(), before any clipping
    rows [21, 25)   sum of their squares
    a step whose done flag is set: the value INCLUDING that step goes to `ep`, `run` restarts from zero
    an explicit reset: `run` of the reset environments is zeroed, `ep` stays

Columns are drones, environment-major: column e * N + i.  Next to the sums the model keeps what the error bound of a float32 / float64
accumulation of the same addends needs (allowed()) and, per environment, the recorded action list that the reference takes np.mean / np.std
of (episode_stats())."""
import numpy as np

RI, ACT, ACT2, COUNT = 17, 17, 21, 25
RAW_MAIN, RAW_QUADCOL = 6, 14
U32, U64 = 2.0 ** -24, 2.0 ** -53          # unit roundoff of the two accumulator formats


class EpisodeSums:
    def __init__(self, E, N):
        self.E, self.N, self.T = E, N, E * N
        z = lambda: np.zeros((COUNT, self.T))       # noqa: E731
        self.run, self.ep = z(), z()
        # for allowed(): sum of max(1, |x_t|) (term rows) / of a_t^2 (square rows), max |partial sum|, steps so far - of the running episode
        # and of the one in `ep`
        self.run_w, self.run_pmax, self.run_n = z(), z(), np.zeros(self.T, dtype=np.int64)
        self.ep_w, self.ep_pmax, self.ep_n = z(), z(), np.zeros(self.T, dtype=np.int64)
        self.run_actions = [[] for _ in range(E)]   # the wrapper's episode_actions list, one per environment
        self.ep_actions = [None] * E
        self.episodes = np.zeros(E, dtype=np.int64)

    # ---- the definition ----------------------------------------------------------------------------------------------------
    def addends(self, actions, rew_info):
        a = np.asarray(actions, dtype=np.float64).reshape(self.T, 4)
        r = np.asarray(rew_info, dtype=np.float64).reshape(self.T, RI)
        return np.concatenate([r.T, a.T, (a * a).T], axis=0)

    def accumulate(self, add, fin):
        """add [25, T], fin bool [T]"""
        v = self.run + add
        self.ep[:, fin] = v[:, fin]
        v[:, fin] = 0.0
        self.run = v

    def step(self, actions, rew_info, done, tol_scale=1.0):
        """tol_scale: this step's term addends are within tol_scale * tol_step * max(1, |x_t|) (allowed()); bookkeeping for the bound only"""
        fin = np.asarray(done).reshape(self.T) != 0
        add = self.addends(actions, rew_info)
        self._track(add, fin, tol_scale)
        a = np.asarray(actions, dtype=np.float64).reshape(self.E, self.N, 4)
        env_fin = fin.reshape(self.E, self.N).any(axis=1)
        for e in range(self.E):
            self.run_actions[e].append(a[e].copy())
            if env_fin[e]:                           # reward_shaping.py:120-121: the list restarts when any agent is done
                self.ep_actions[e], self.run_actions[e] = self.run_actions[e], []
                self.episodes[e] += 1
        self.accumulate(add, fin)

    def reset(self, env_mask=None):
        m = np.ones(self.E, dtype=bool) if env_mask is None else np.asarray(env_mask).reshape(self.E) != 0
        cols = np.repeat(m, self.N)
        self.zero_run(cols)
        self.run_w[:, cols] = 0.0
        self.run_pmax[:, cols] = 0.0
        self.run_n[cols] = 0
        for e in np.nonzero(m)[0]:
            self.run_actions[e] = []

    def zero_run(self, cols):
        self.run[:, cols] = 0.0

    # ---- bookkeeping for the bound --------------------------------------------------------------------------------------------
    def _track(self, add, fin, tol_scale=1.0):
        w = np.zeros_like(add)
        w[:RI] = tol_scale * np.maximum(1.0, np.abs(add[:RI]))
        w[ACT2:] = add[ACT2:]
        partial = self.run + add
        self.run_w += w
        self.run_pmax = np.maximum(self.run_pmax, np.abs(partial))
        self.run_n += 1
        for dst, src in ((self.ep_w, self.run_w), (self.ep_pmax, self.run_pmax)):
            dst[:, fin] = src[:, fin]
            src[:, fin] = 0.0
        self.ep_n[fin] = self.run_n[fin]
        self.run_n[fin] = 0

    def allowed(self, which, tol_step, u):
        """|device - model| allowed per element of `run` / `ep` ([25, T]) for an accumulation in a format of unit roundoff `u` whose term
        addends are within tol_step * max(1, |x_t|) of the model's:

            sum_t tol_step * max(1, |x_t|)  +  (n - 1) * u * max_t |partial_t|

        the action rows have exact addends (tol_step = 0), the square rows one rounding of a_t^2 per step (u * a_t^2).  A step that was given a
        tol_scale counts with tol_scale * tol_step."""
        w, pmax, n = (self.run_w, self.run_pmax, self.run_n) if which == "run" else (self.ep_w, self.ep_pmax, self.ep_n)
        out = np.maximum(n - 1, 0)[None, :] * u * pmax
        out[:RI] += tol_step * w[:RI]
        out[ACT2:] += u * w[ACT2:]
        return out


def allowed(model, which, tol_step, u):
    return model.allowed(which, tol_step, u)


def episode_stats(ep, steps, err=None):
    """One environment's finished episode as reward_shaping.py:79-106 reports it.  ep: [25, N] sums; steps: the recorded list of the [N, 4]
    actions of the episode's steps.  Returns true_reward [N], rew [17, N] (row RAW_MAIN replaced by true_reward, :86), mean [4] and std [4]
    of every action component pooled over agents and steps - np.mean / np.std of the list, as the reference does, not the moment formula.
    err: [25, N] bound on the sums -> also the same bound pushed through the formulas: true_reward linear, mean linear, variance
    err(a2) + 2 |a1| err(a1), std that over 2 std."""
    ep = np.asarray(ep, dtype=np.float64)
    true_reward = ep[RAW_MAIN] + 1000.0 * ep[RAW_QUADCOL]
    rew = ep[:RI].copy()
    rew[RAW_MAIN] = true_reward
    acts = np.array(steps).transpose()                      # [4, N, steps] (reward_shaping.py:100-101)
    mean = np.array([np.mean(acts[k]) for k in range(4)])
    std = np.array([np.std(acts[k]) for k in range(4)])
    out = dict(true_reward=true_reward, rew=rew, mean=mean, std=std)
    if err is not None:
        count = acts.shape[1] * acts.shape[2]
        e_true = err[RAW_MAIN] + 1000.0 * err[RAW_QUADCOL]
        e_rew = err[:RI].copy()
        e_rew[RAW_MAIN] = e_true
        e_a1 = err[ACT:ACT2].sum(axis=1) / count
        e_a2 = err[ACT2:COUNT].sum(axis=1) / count
        e_var = e_a2 + 2.0 * np.abs(mean) * e_a1
        out["err"] = dict(true_reward=e_true, rew=e_rew, mean=e_a1, var=e_var, std=e_var / (2.0 * std))
    return out
