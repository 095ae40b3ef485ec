"""The cases of tests/test_encoder_epilogues_gpu.py as plain data (nothing here needs a GPU or the library), shared with
tests/test_sampler_model_cpu.py, which checks without a GPU that CONFIGS reaches every kernel of the encoder's table and that the sampler
inputs separate the model from its mutants under the bound the GPU tests apply."""
from collections import namedtuple

MEAN_EMBED, ATTENTION, MLP, NONE, MHA, S2R = range(6)    # qs_enc_params.nbr_encoder (policy.MODELS)

# precision: 0 bf16 / 1 reference precision (fp16 pairs); wide: qs_enc_set_wide_min(1) (every batch on the 32-agent workgroups) or (0) (never);
# pingpong: qs_enc_set_pingpong; kernels: what the forward pass is meant to launch, qs_encoder_<name>_kernel ("" = qs_encoder_kernel)
Config = namedtuple("Config", "name precision model num_nbr obst_dim pingpong wide kernels")

CONFIGS = [
    Config("main_mean_embed", 0, MEAN_EMBED, 6, 0, 1, 0, [""]),
    Config("main_mean_embed_obst", 0, MEAN_EMBED, 2, 9, 1, 0, [""]),
    Config("main_mlp", 0, MLP, 6, 0, 1, 0, [""]),
    Config("main_no_encoder", 0, NONE, 6, 9, 1, 0, [""]),
    Config("attention", 0, ATTENTION, 6, 0, 1, 0, ["embed", "attn"]),
    Config("mha", 0, MHA, 2, 9, 1, 0, ["mha"]),
    Config("s2r", 0, S2R, 2, 9, 1, 0, ["s2r"]),
    Config("split_mean_embed", 1, MEAN_EMBED, 6, 0, 1, 0, ["split"]),
    Config("split_attention", 1, ATTENTION, 5, 9, 1, 0, ["embed_split", "attn_split"]),
    Config("split_mha", 1, MHA, 2, 9, 1, 0, ["mha_split"]),
    Config("split_s2r", 1, S2R, 2, 9, 1, 0, ["s2r_split"]),
    Config("wide1", 0, MEAN_EMBED, 1, 0, 0, 1, ["wide1"]),
    Config("wide2", 0, MEAN_EMBED, 4, 9, 0, 1, ["wide2"]),
    Config("wide3", 0, MEAN_EMBED, 6, 0, 0, 1, ["wide3"]),
    Config("pp1", 0, MEAN_EMBED, 2, 0, 1, 1, ["pp1"]),
    Config("pp2", 0, MEAN_EMBED, 4, 0, 1, 1, ["pp2"]),
    Config("pp3", 0, MEAN_EMBED, 6, 0, 1, 1, ["pp3"]),
    Config("pp1o", 0, MEAN_EMBED, 2, 9, 1, 1, ["pp1o"]),
    Config("pp2o", 0, MEAN_EMBED, 4, 9, 1, 1, ["pp2o"]),
    Config("pp3o", 0, MEAN_EMBED, 5, 9, 1, 1, ["pp3o"]),
    Config("attention_wide1", 0, ATTENTION, 1, 0, 1, 1, ["embed_wide1", "attn_wide1"]),
    Config("attention_wide2", 0, ATTENTION, 2, 9, 1, 1, ["embed_wide2", "attn_wide2"]),
    Config("attention_wide3", 0, ATTENTION, 6, 0, 1, 1, ["embed_wide3", "attn_wide3"]),
]

# (B, head_dim): 33 = two or three workgroups with a one-row tail, 32 fills the workgroups exactly, 1 is the smallest batch
SHAPES = [(33, 4), (33, 8), (1, 3), (32, 1)]
# ... and one batch at which the uniforms reach far enough into the tail of ua (32836 draws of ua: down to ~3e-5) for the sampler's "+ 0.5" to
# show above the bound, on one 16-agent and one 32-agent kernel: 514 / 257 workgroups with a one-row tail
TAIL_SHAPE = (8209, 8)
TAIL_CONFIGS = ("main_mean_embed", "pp3")

SENTINEL_ROWS = 3

# the standard deviations of the sampler cases: exp(log_std[h]) for the first head_dim entries (two orders of magnitude apart, one above 1)
SIGMAS = [0.5, 0.25, 1.0, 0.1, 2.0, 0.05, 0.75, 0.3]
# no mean of a sampler case is larger than this (asserted by every GPU case): what lets the CPU test evaluate the GPU bound without the means
HEAD_ABS_MAX = 16.0


def sampler_inputs_of(config_index, shape_index):
    """(seed, counter, step) of a forward pass of the matrix: every case its own 64-bit seed (both halves non-zero), counter and step"""
    n = 1 + len(SHAPES) * config_index + shape_index
    return (0x9E3779B97F4A7C15 * n) & 0xFFFFFFFFFFFFFFFF, 1000 * config_index + 7 * shape_index + 1, (config_index + shape_index) % 5


# counter semantics (bit for bit from the kernel; the model is evaluated at the summed value): name -> (seed, counter as the int32 tensor holds
# it, step, and the (counter, step) pair that has to give the same bits, or None)
COUNTER_SHAPE = (33, 8)
COUNTER_CONFIGS = ("main_mean_embed", "wide3")
COUNTER_CASES = {
    "counter_plus_step": (0x1234567811, 7, 3, (10, 0)),
    "int32_minus_one_wraps": (0x1234567811, -1, 2, (1, 0)),
    "seed_high_word": (0xC0FFEE1100000005, 10, 0, None),
    "seed_zero_low_word": (0xABCDEF0100000000, 10, 0, None),
    "seed_zero_high_word": (0x00000000DEADBEEF, 10, 0, None),
}

# qs_rollout_pre / qs_rollout_post called directly
PRE_AGENTS = [1, 5, 257, 2048 * 256 + 3]      # the last: more agents than 2048 blocks of 256 threads - the grid-stride loop runs
PRE_SEED, PRE_COUNTER = 0x0F1E2D3C4B5A6978, 0x7FFFFFFE
PRE_OBS_COUNTS = [0, 3, 4, 270, 2 ** 21 + 5]
POST_AGENTS = [1, 257, 2048 * 256 + 3]

# closed loop: 4 environments x 8 agents, 6 steps per segment, three run()s; the constructor's warm-up step leaves the counter at 1
LOOP_ENVS, LOOP_AGENTS, LOOP_STEPS, LOOP_RUNS, LOOP_SEED, LOOP_COUNTER0 = 4, 8, 6, 3, 11, 1

SamplerInput = namedtuple("SamplerInput", "site seed counter step agents head_dim")   # site: "epilogue" (sample_action) or "pre" (qs_rollout_pre_kernel)


def sampler_inputs():
    """every (seed, counter, step, B, head_dim) a GPU test compares with the model, with the code site that draws it"""
    out = []
    names = [c.name for c in CONFIGS]
    for i in range(len(CONFIGS)):
        for j, (B, hd) in enumerate(SHAPES):
            out.append(SamplerInput("epilogue", *sampler_inputs_of(i, j), B, hd))
    for name in TAIL_CONFIGS:
        out.append(SamplerInput("epilogue", *sampler_inputs_of(names.index(name), len(SHAPES)), *TAIL_SHAPE))
    for seed, counter, step, _ in COUNTER_CASES.values():
        out.append(SamplerInput("epilogue", seed, counter & 0xFFFFFFFF, step, *COUNTER_SHAPE))
    for A in PRE_AGENTS:
        out.append(SamplerInput("pre", PRE_SEED, PRE_COUNTER, 0, A, 4))
    for r in range(LOOP_RUNS):
        for t in range(LOOP_STEPS):
            out.append(SamplerInput("epilogue", LOOP_SEED, LOOP_COUNTER0 + LOOP_STEPS * r, t, LOOP_ENVS * LOOP_AGENTS, 4))    # in place: counter + step
            out.append(SamplerInput("pre", LOOP_SEED, LOOP_COUNTER0 + LOOP_STEPS * r + t, 0, LOOP_ENVS * LOOP_AGENTS, 4))      # copying: one counter per step
    return out
