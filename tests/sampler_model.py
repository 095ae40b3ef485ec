"""The Gaussian action sampler of the rollout (sample_action in csrc/qs_enc_device.h, qs_rollout_pre_kernel in csrc/qs_rollout_glue.inc) as a
specification: numpy, integers in uint64, floats in float64, nothing imported from the project (DESIGN.md 8b carries the same paragraph).

Philox.  philox4x32_10(c[..., 4], k[..., 2]) is the standard Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
SC11; Random123), vectorised over leading axes.  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments 0x9E3779B9 (k0) and 0xBB67AE85
(k1) after every round; one round maps (c0, c1, c2, c3) to [hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)]; ten rounds.

Draw of head component h of agent a.  Counter words (a, (counter + step) mod 2^32, 0x51, h >> 2); key (seed & 0xffffffff, seed >> 32); output
words w[0..3].  Pair p = (h >> 1) & 1;  ua = ((w[2p] >> 9) + 0.5) / 2^23;  ub = ((w[2p+1] >> 9) + 0.5) / 2^23  (both strictly inside (0, 1));
z = sqrt(-2 ln ua) * (cos if h is even else sin)(2 pi ub);  action = mean + exp(log_std[h]) * z.

qs_rollout_pre is the head_dim == 4, step == 0 case of the same definition.

`mutant` names ONE deliberate deviation from the definition (MUTANTS): what tests/test_sampler_model_cpu.py uses to show that the bound of the
GPU tests separates the definition from its plausible mis-implementations on the very inputs those tests run."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM = 0x51

MUTANTS = ("sincos_swapped", "pairs_swapped", "shift_8", "no_half", "step_ignored", "agent_mod_16", "agent_mod_32", "group_zero",
           "key_halves_swapped", "nine_rounds")


def philox4x32_10(counter, key, rounds=10):
    """counter [..., 4], key [..., 2] (any integer type, values < 2^32) -> [..., 4] uint64 holding the four 32-bit output words"""
    c = np.asarray(counter).astype(np.uint64) & np.uint64(MASK)
    k = np.asarray(key).astype(np.uint64) & np.uint64(MASK)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    lo, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo, (p0 >> sh) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + np.uint64(W0)) & lo, (k1 + np.uint64(W1)) & lo
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def uniforms(seed, counter, step, agents, head_dim, mutant=None):
    """(ua, ub), [agents, head_dim] float64 each: the two uniforms behind component h of agents 0 .. agents - 1"""
    assert mutant is None or mutant in MUTANTS
    a = np.arange(agents, dtype=np.uint64)[:, None]
    h = np.arange(head_dim, dtype=np.uint64)[None, :]
    if mutant == "agent_mod_16":
        a = a % np.uint64(16)
    if mutant == "agent_mod_32":
        a = a % np.uint64(32)
    ctr = (int(counter) + (0 if mutant == "step_ignored" else int(step))) & MASK
    group = np.zeros_like(h) if mutant == "group_zero" else h >> np.uint64(2)
    c = np.stack(np.broadcast_arrays(a, np.uint64(ctr), np.uint64(STREAM), group), axis=-1)
    k = [int(seed) & MASK, (int(seed) >> 32) & MASK]
    if mutant == "key_halves_swapped":
        k = k[::-1]
    w = philox4x32_10(c, np.array(k, dtype=np.uint64), rounds=9 if mutant == "nine_rounds" else 10)      # [agents, head_dim, 4]
    p = (h >> np.uint64(1)) & np.uint64(1)
    if mutant == "pairs_swapped":
        p = np.uint64(1) - p
    p = np.broadcast_to(p, w.shape[:2]).astype(np.int64)
    wa = np.take_along_axis(w, (2 * p)[..., None], axis=-1)[..., 0]
    wb = np.take_along_axis(w, (2 * p + 1)[..., None], axis=-1)[..., 0]
    shift = np.uint64(8 if mutant == "shift_8" else 9)
    half = 0.0 if mutant == "no_half" else 0.5
    to_u = lambda x: ((x >> shift).astype(np.float64) + half) / 8388608.0
    return to_u(wa), to_u(wb)


def normals(seed, counter, step, agents, head_dim, mutant=None):
    """z [agents, head_dim] float64: the standard normal draws of one forward pass (a mutant may give nan / inf where the definition cannot)"""
    ua, ub = uniforms(seed, counter, step, agents, head_dim, mutant)
    even = (np.arange(head_dim) % 2 == 0)[None, :]
    if mutant == "sincos_swapped":
        even = ~even
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(-2.0 * np.log(ua))
        return r * np.where(even, np.cos(2.0 * np.pi * ub), np.sin(2.0 * np.pi * ub))


def actions(mean, log_std, seed, counter, step=0, mutant=None):
    """mean [agents, head_dim], log_std [head_dim] -> mean + exp(log_std) * z in float64"""
    mean = np.asarray(mean, dtype=np.float64)
    return mean + np.exp(np.asarray(log_std, dtype=np.float64))[None, :] * normals(seed, counter, step, mean.shape[0], mean.shape[1], mutant)


def bound(head_out, sigma, z, z_tol):
    """what a float32 evaluation with fast log / sincos / exp may differ by from actions(): sigma * z_tol for the intrinsics (a measured
    constant, tests/encoder_epilogue_cases.py: fast log, sincos, exp and the roundings inside z) + 2^-23 * (|head_out| + sigma * |z|): the
    product sigma * z rounded to float32 (2^-24 sigma |z|) and the sum with the mean rounded to float32 (2^-24 of at most |mean| + sigma |z|),
    together 2^-24 (|mean| + 2 sigma |z|) <= the term."""
    head_out, sigma, z = np.abs(np.asarray(head_out, dtype=np.float64)), np.asarray(sigma, dtype=np.float64), np.abs(np.asarray(z, dtype=np.float64))
    return sigma * z_tol + 2.0 ** -23 * (head_out + sigma * z)
