"""What the host decides about a forward pass of the policy encoder (csrc/qs_enc_plan.h), without a GPU: the header is compiled alone with the
host compiler, and the kernels it picks - with their grid divisor, LDS bytes and `out` argument - are compared with the rule restated here
(DESIGN.md 10).  The GPU tests cannot see a mistake in that rule: the ping-pong and lock-step kernels agree bit for bit by design, and a
kernel built for three neighbours per pass computes the right features for two."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quad-swarm-rl_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include "qs_enc_plan.h"
#define ROW(sym, lds, agents, has_out) {nullptr, #sym, lds, agents, has_out},
static const EncKernel table[ENC_NUM_KERNELS] = {ENC_KERNELS(ROW)};
int main() {
    printf("layout main %d\nlayout attention %d\nlayout embed %d\nlayout multi-head %d\nlayout wide %d\nlayout embed-wide %d\n"
           "layout attention-wide %d\nlayout split %d\nlayout split+scores %d\nsplane %d\n",
           EncLdsMain::bytes, EncLdsAttn::bytes, EncLdsEmbed::bytes, EncLdsMha::bytes, EncLdsWide::bytes, EncLdsEmbedWide::bytes,
           EncLdsAttnWide::bytes, EncLdsSplit::bytes, EncLdsSplit::bytes_scores, ENC_SPLANE);
    for (const EncKernel &k : table) printf("kernel %s %d %d %d\n", k.name, k.lds_bytes, k.agents, k.has_out);
    const int thresholds[2] = {0, 100}, batches[2] = {99, 100}, obst[2] = {0, 9};
    for (int precision = 0; precision < 2; ++precision)
        for (int model = 0; model < 6; ++model)
            for (int K = 0; K <= 8; ++K)
                for (int od : obst)
                    for (int pp = 0; pp < 2; ++pp)
                        for (int thr : thresholds)
                            for (int B : batches) {
                                const EncPlan p = enc_select(model, K, od, precision, B, thr, pp);
                                printf("select %d %d %d %d %d %d %d", precision, model, K, od, pp, thr, B);
                                for (int i = 0; i < p.n; ++i) {
                                    const EncKernel &k = table[p.kernel[i]];
                                    printf(" %s %d %d %d", k.name, k.agents, k.lds_bytes, k.has_out);
                                }
                                printf("\n");
                            }
    return 0;
}
"""

# dynamic LDS bytes of every layout: the parent's formulas, the exported ones read back from its library (qs_enc_lds_bytes, _of, _split)
LAYOUTS = {"main": 79872, "attention": 79616, "embed": 52480, "multi-head": 125184, "wide": 145408, "embed-wide": 90624,
           "attention-wide": 159232, "split": 159744, "split+scores": 161280}

# kernel -> (layout, agents per workgroup, takes `out`)
KERNELS = {"qs_encoder_kernel": ("main", 16, 1), "qs_encoder_embed_kernel": ("embed", 16, 0), "qs_encoder_attn_kernel": ("attention", 16, 1),
           "qs_encoder_mha_kernel": ("multi-head", 16, 1), "qs_encoder_s2r_kernel": ("multi-head", 16, 1),
           "qs_encoder_split_kernel": ("split", 16, 1), "qs_encoder_embed_split_kernel": ("split", 16, 0),
           "qs_encoder_attn_split_kernel": ("split+scores", 16, 1), "qs_encoder_mha_split_kernel": ("split", 16, 1),
           "qs_encoder_s2r_split_kernel": ("split", 16, 1)}
for _w in "123":
    KERNELS[f"qs_encoder_wide{_w}_kernel"] = KERNELS[f"qs_encoder_pp{_w}_kernel"] = KERNELS[f"qs_encoder_pp{_w}o_kernel"] = ("wide", 32, 1)
    KERNELS[f"qs_encoder_embed_wide{_w}_kernel"] = ("embed-wide", 32, 0)
    KERNELS[f"qs_encoder_attn_wide{_w}_kernel"] = ("attention-wide", 32, 1)

MEAN_EMBED, ATTENTION, MLP, NONE, MHA, S2R = range(6)


def expected(precision, model, K, obst_dim, pp, threshold, B):
    """the selection rule: the first branch that matches"""
    att = model == ATTENTION and K > 0
    if precision == 1:
        if model == S2R:
            return ["s2r_split"]
        if model == MHA:
            return ["mha_split"]
        return ["embed_split", "attn_split"] if att else ["split"]
    if threshold > 0 and B >= threshold and K > 0 and (model == MEAN_EMBED or att):
        w = 1 if K == 1 else (2 if K in (2, 4) else 3)
        if att:
            return [f"embed_wide{w}", f"attn_wide{w}"]
        if pp and K in (2, 4, 5, 6):
            return [f"pp{-(-K // 2)}" + ("o" if obst_dim > 0 else "")]
        return [f"wide{w}"]
    if model == S2R:
        return ["s2r"]
    if model == MHA:
        return ["mha"]
    return ["embed", "attn"] if att else [""]


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "a host C++ compiler (the code-object checker is built with one)"
    tmp = tmp_path_factory.mktemp("enc_select")
    src, exe = tmp / "enc_select.cpp", tmp / "enc_select"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


def test_every_layout_asks_for_the_bytes_it_always_did(program_output):
    got = {line.split()[1]: int(line.split()[2]) for line in program_output if line.startswith("layout ")}
    assert got == LAYOUTS
    (splane,) = [int(line.split()[1]) for line in program_output if line.startswith("splane ")]
    assert 2 * splane == LAYOUTS["main"] and 4 * splane == LAYOUTS["split"]   # one plane = the largest 16-agent layout, in 2-byte elements


def test_the_kernel_list_names_each_kernel_once_with_its_layout(program_output):
    rows = [line.split()[1:] for line in program_output if line.startswith("kernel ")]
    assert sorted(r[0] for r in rows) == sorted(KERNELS) and len(rows) == 25
    for name, lds, agents, has_out in rows:
        layout, want_agents, want_out = KERNELS[name]
        assert (int(lds), int(agents), int(has_out)) == (LAYOUTS[layout], want_agents, want_out), name


def test_selection_follows_the_rule_and_reaches_every_kernel(program_output):
    lines = [line.split() for line in program_output if line.startswith("select ")]
    combos = list(itertools.product((0, 1), range(6), range(9), (0, 9), (0, 1), (0, 100), (99, 100)))
    assert [tuple(int(x) for x in f[1:8]) for f in lines] == combos
    chosen = set()
    for f, combo in zip(lines, combos):
        got = [(f[i], int(f[i + 1]), int(f[i + 2]), int(f[i + 3])) for i in range(8, len(f), 4)]
        want = []
        for middle in expected(*combo):
            name = f"qs_encoder{'_' if middle else ''}{middle}_kernel"
            layout, agents, has_out = KERNELS[name]
            want.append((name, agents, LAYOUTS[layout], has_out))
        assert got == want, combo
        chosen.update(name for name, *_ in got)
    assert chosen == set(KERNELS)
