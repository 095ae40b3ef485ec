"""The attention weights of the policy encoders, on the device (include/quadswarm_attention.h states the semantics; csrc/qs_attn_weights.inc).

Three of the reference's encoder classes decide by attention what an agent looks at: QuadNeighborhoodEncoderAttention
(swarm_rl/models/quad_multi_model.py:44-101, a softmax over the K neighbour slots), QuadMultiHeadAttentionEncoder (:124-196, 4 heads over the
token pair [neighbour embedding, obstacle embedding]) and QuadSingleHeadAttentionEncoder_Sim2Real (:199-248, one head over the same pair).  The
reference computes those weights and drops them (:191); the figure of its paper on them (paper/attn_heatmap.py: a drone-by-drone matrix of
weights, and the same with the neighbours' velocities zeroed) has its numbers typed in by hand.  The fused forward kernels compute the same
softmaxes and keep them in registers.  `AttentionProbe` is a launch of its own that stores them - for every agent of every running
environment, without leaving the device and without running the torch module under hooks.  It produces the numbers, not the picture.
"""
import ctypes as C

from . import abi, native, policy
from .abi import EncLayer, EncParams

ROW_SHAPES = {abi.QS_ENC_MODEL_MHA: (4, 2, 2), abi.QS_ENC_MODEL_S2R: (2, 2)}   # attention: (num_nbr,)


def _model_of(module):
    """QS_ENC_* of a restatement module (policy.make_reference_*), or NotImplementedError for one without attention / at a width that is not built"""
    kind = getattr(module, "nbr_encoder", "mean_embed")
    if kind not in ("attention", "multi_head_attention", "single_head_sim2real"):
        raise NotImplementedError(f"AttentionProbe: a {kind!r} encoder computes no attention weights (attention, multi_head_attention and "
                                  f"single_head_sim2real do)")
    model = policy.MODELS.index(kind)
    if model == abi.QS_ENC_NBR_ATTENTION:
        widths = {module.neighbor_encoder[0].out_features, module.neighbor_encoder[2].out_features, module.attention_mlp[0].out_features,
                  module.attention_mlp[2].out_features}
    else:
        att = module.attention_layer
        heads = att.w_qs.out_features // att.w_qs.in_features
        widths = {lin.out_features for seq in (module.neighbor_encoder, module.obstacle_encoder) for lin in seq if hasattr(lin, "out_features")}
        widths |= {att.w_qs.in_features, att.w_qs.out_features // heads, att.w_ks.out_features // heads}
    narrow = model == abi.QS_ENC_MODEL_S2R and len(widths) == 1 and next(iter(widths)) in policy.NARROW_WIDTHS
    if (widths != {policy.HIDDEN} and not narrow) or getattr(module, "nonlinearity", "tanh") != "tanh":
        raise NotImplementedError(f"AttentionProbe covers the widths of the fused encoder kernels: {policy.HIDDEN} with tanh for every class and "
                                  f"{policy.NARROW_WIDTHS} for the Sim2Real class; got widths {sorted(widths)}, nonlinearity "
                                  f"{getattr(module, 'nonlinearity', 'tanh')!r}, class {kind!r}")
    return model


class AttentionProbe:
    """AttentionProbe(module).weights(obs[B, D] float32 on the GPU) -> the attention weights `module` computes on those rows, float32:
    [B, K] for the attention neighbour encoder (the softmax over the K neighbour slots, in the slot order of the row), [B, 4, 2, 2] for the
    multi-head class (head, query token, key token; token 0 = neighbour embedding, token 1 = obstacle embedding), [B, 2, 2] for the Sim2Real
    class (width 256 and policy.NARROW_WIDTHS).  `row_shape` is that shape without B.

    module: one of policy.make_reference_encoder(nbr_encoder="attention") / make_reference_mha_encoder / make_reference_sim2real_encoder, e.g.
    from policy.encoder_from_state_dict; anything else raises NotImplementedError.  The probe packs its OWN weights in reference precision
    (fp16 pairs, policy.pack_linear(split=True)) whatever precision the sampler's FusedQuadEncoder runs in: a diagnostic should not differ
    from the fp32 learner by the 1e-2 of the bf16 path; the weights come out within 1e-5 of the fp32 module.  refresh() re-reads the module.

    The attention neighbour encoder pairs rows ACROSS the batch (quad_multi_model.py:84,92 tile the whole batch: slot k of agent a meets the
    self observation and the mean embedding of agent (a*K + k) mod B), so its weights are those of the module on `obs` as ONE batch, exactly
    as the forward pass's features are.  Its two scratch buffers are allocated on the first call and again only when the batch grows
    (`scratch=` a reference-precision FusedQuadEncoder of the same module: that encoder's buffers are used instead - a forward pass fills them
    again before it reads them).  Later calls allocate nothing but an `out` that was not passed, launch on the current stream and record into
    a HIP graph."""

    def __init__(self, module, device=0, scratch=None):
        import torch
        self._torch = torch
        model = _model_of(module)
        if not torch.cuda.is_available():
            raise native.QsError("AttentionProbe needs a GPU: there is no CPU fallback (attention_weights_reference is the torch statement)")
        self.module, self.device = module, torch.device("cuda", device)
        self._packed, self._raw, self._a3 = [], [], None

        def layer(linear, cols=None):
            w, b, M, K = policy.pack_linear(linear, self.device, cols, split=True)
            self._packed.append((linear, cols, w, b))
            return EncLayer(w.data_ptr(), b.data_ptr(), M, K)

        P = EncParams()
        P.self_dim, P.nbr_dim, P.num_nbr, P.obst_dim = module.self_dim, module.nbr_dim, module.num_nbr, module.obst_dim
        P.obs_dim = module.self_dim + module.nbr_dim * module.num_nbr + module.obst_dim
        P.nbr_encoder, P.precision = model, 1
        self.attention = model == abi.QS_ENC_NBR_ATTENTION
        if self.attention:
            if module.self_dim + module.nbr_dim > 32:
                raise ValueError("attention encoder: self_dim + nbr_dim must fit one 32-wide K step")
            P.n1, P.n2 = layer(module.neighbor_encoder[0]), layer(module.neighbor_encoder[2])
            P.a1e, P.a1m = layer(module.attention_mlp[0], (0, policy.HIDDEN)), layer(module.attention_mlp[0], (policy.HIDDEN, 2 * policy.HIDDEN))
            P.a2 = layer(module.attention_mlp[2])
            a3 = module.attention_mlp[4]   # 256 -> 1: fp32 weight row, the bias in the struct
            a3w = a3.weight.detach().float().reshape(-1).to(self.device).clone()   # (a copy of its own, as the packed layers are: refresh() is what moves it)
            self._raw.append((lambda: a3.weight.reshape(-1), a3w))
            self._a3 = a3
            P.a3w, P.a3b = a3w.data_ptr(), float(a3.bias.detach().float().item())
            self.row_shape = (module.num_nbr,)
        else:
            if module.nbr_dim * module.num_nbr > 64:
                raise ValueError("multi-head attention encoder: num_nbr * nbr_dim must fit two 32-wide K steps")
            P.n1, P.o1 = layer(module.neighbor_encoder[0]), layer(module.obstacle_encoder[0])
            if model == abi.QS_ENC_MODEL_MHA:
                P.n2, P.o2 = layer(module.neighbor_encoder[2]), layer(module.obstacle_encoder[2])
            P.mq, P.mk = layer(module.attention_layer.w_qs), layer(module.attention_layer.w_ks)
            self.row_shape = ROW_SHAPES[model]
        if scratch is not None and not (self.attention and getattr(scratch, "attention", False) and scratch._split
                                        and scratch.params.num_nbr == P.num_nbr and scratch.device == self.device):
            raise ValueError("scratch=: a FusedQuadEncoder(precision='fp32') of an attention module with the same number of neighbours, on the same device")
        self._shared, self._scratch_rows = scratch, 0
        self.params = P
        self._elems = policy.lib().qs_attn_row_elems(C.byref(P))
        if self._elems < 0:
            raise native.QsError(f"qs_attn_row_elems refused the module ({self._elems}): {policy.lib().qs_enc_last_error().decode()}")
        n = 1
        for d in self.row_shape:
            n *= d
        assert n == self._elems, (self.row_shape, self._elems)

    def refresh(self):
        """Re-read the module's weights INTO the buffers the kernels - and any captured HIP graph - already point at.  The last score layer's
        bias of the attention neighbour encoder lives in the parameter struct (a3b): a graph captured before keeps the old value of that one
        scalar until it is recaptured."""
        for linear, cols, w, b in self._packed:
            nw, nb, _, _ = policy.pack_linear(linear, self.device, cols, split=True)
            w.copy_(nw)
            b.copy_(nb)
        for src, dst in self._raw:
            dst.copy_(src().detach().float().reshape(dst.shape))
        if self._a3 is not None:
            self.params.a3b = float(self._a3.bias.detach().float().item())

    def _scratch(self, B):
        """attention only: e_i [B*K, 2, 256] fp16 planes and W_m e_mean [B, 256] fp32, handed from the first launch to the second (the
        buffers of policy.FusedQuadEncoder._scratch in reference precision)"""
        if not self.attention:
            return
        if self._shared is not None:
            self._shared._scratch(B)
            self.params.ebuf, self.params.gbuf = self._shared.params.ebuf, self._shared.params.gbuf
        elif B > self._scratch_rows:
            torch = self._torch
            self._ebuf = torch.empty((B * self.params.num_nbr, 2 * policy.HIDDEN), device=self.device, dtype=torch.bfloat16)
            self._gbuf = torch.empty((B, policy.HIDDEN), device=self.device, dtype=torch.float32)
            self.params.ebuf, self.params.gbuf = self._ebuf.data_ptr(), self._gbuf.data_ptr()
            self._scratch_rows = B

    def weights(self, obs, out=None):
        torch = self._torch
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.dim() == 2 and obs.shape[1] == self.params.obs_dim
        B = obs.shape[0]
        if out is None:
            out = torch.empty((B,) + self.row_shape, device=obs.device, dtype=torch.float32)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B,) + self.row_shape
        self._scratch(B)
        rc = policy.lib().qs_attn_weights(obs.data_ptr(), B, C.byref(self.params), out.data_ptr(), C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
        if rc != 0:
            raise native.QsError(f"qs_attn_weights failed ({rc}): {policy.lib().qs_enc_last_error().decode()}")
        return out

    __call__ = weights


def attention_weights_reference(module, obs):
    """The same numbers from the torch module, in the module's dtype (float64 when the module was cast with .double()): [B, K], [B, 4, 2, 2] or
    [B, 2, 2].  Restates quad_multi_model.py:77-100 and attention_layer.py:29-44 / :73-84 on the restatement modules' layers; their forward() is
    not touched.  NotImplementedError for a module without attention."""
    import torch
    kind = getattr(module, "nbr_encoder", "mean_embed")
    B = obs.shape[0]
    nb = module.nbr_dim * module.num_nbr
    with torch.no_grad():
        if kind == "attention":                                                 # :77-100, including what .repeat() pairs up
            K = module.num_nbr
            nbrs = obs[:, module.self_dim:module.self_dim + nb].reshape(-1, module.nbr_dim)
            e = module.neighbor_encoder(torch.cat((obs[:, :module.self_dim].repeat(K, 1), nbrs), dim=1))
            e_mean = e.reshape(B, -1, e.shape[-1]).mean(dim=1)
            alpha = module.attention_mlp(torch.cat((e, e_mean.repeat(K, 1)), dim=1)).view(B, -1)
            return torch.softmax(alpha, dim=1)
        if kind not in ("multi_head_attention", "single_head_sim2real"):
            raise NotImplementedError(f"attention_weights_reference: a {kind!r} encoder computes no attention weights")
        att = module.attention_layer
        x = torch.stack((module.neighbor_encoder(obs[:, module.self_dim:module.self_dim + nb]), module.obstacle_encoder(obs[:, module.self_dim + nb:])), dim=1)
        d = att.w_qs.in_features
        if kind == "single_head_sim2real":                                      # attention_layer.py:73-84
            q, k = att.w_qs(x), att.w_ks(x)
            return torch.softmax(torch.matmul(q / d ** 0.5, k.transpose(-1, -2)), dim=-1)
        heads = att.w_qs.out_features // d                                      # attention_layer.py:29-44, :102-108
        q = att.w_qs(x).view(B, 2, heads, d).transpose(1, 2)
        k = att.w_ks(x).view(B, 2, heads, d).transpose(1, 2)
        return torch.softmax(torch.matmul(q / d ** 0.5, k.transpose(2, 3)), dim=-1)


def zero_neighbor_velocity(obs, self_dim, num_nbr, nbr_dim=6):
    """A copy of the rows with the relative velocity of every neighbour slot - columns self_dim + nbr_dim*k + 3 .. + 5 - set to zero: the second
    panel of the reference's figure (paper/attn_heatmap.py, "velocities zeroed").  torch tensor or numpy array."""
    out = obs.clone() if hasattr(obs, "clone") else obs.copy()
    for k in range(num_nbr):
        c = self_dim + nbr_dim * k + 3
        out[:, c:c + 3] = 0
    return out


def attention_matrix(w, num_agents, ids=None):
    """[E*N, K] weights of the attention neighbour encoder -> [E, N, N] drone-by-drone matrices with a zero diagonal: entry (i, j) is the weight
    drone i gives drone j.  torch tensor or numpy array.

    Without `ids` this is valid only when every drone sees ALL others (K == N - 1): the slots of drone i are then the other drones in index order
    (gym_art/quadrotor_multi/quadrotor_multi.py:247-274); ValueError otherwise.  With fewer slots the environment picks the nearest, and `ids` says
    which: int32 [E*N, K] from native.Stepper.neighbor_ids / BatchedQuadSwarm.neighbor_ids for the rows the weights were computed on
    (include/quadswarm_neighbors.h) - any 1 <= K <= N - 1 then; slots whose id is -1 are dropped.  Device tensors (float32 weights) go through
    qs_neighbor_scatter, one launch on the current stream; numpy arrays and host tensors through a host loop with the same definition."""
    N = int(num_agents)
    if ids is not None:
        return _attention_matrix_ids(w, N, ids)
    if w.ndim != 2 or N < 2 or w.shape[1] != N - 1 or w.shape[0] % N != 0:
        raise ValueError(f"attention_matrix: weights [E * {N}, {N - 1}] wanted (every drone sees all others), got {tuple(w.shape)}")
    E = w.shape[0] // N
    w = w.reshape(E, N, N - 1)
    if hasattr(w, "new_zeros"):
        out = w.new_zeros((E, N, N))
    else:
        import numpy as np
        out = np.zeros((E, N, N), dtype=w.dtype)
    for i in range(N):
        out[:, i, :i] = w[:, i, :i]
        out[:, i, i + 1:] = w[:, i, i:]
    return out


def _attention_matrix_ids(w, N, ids):
    import numpy as np
    if w.ndim != 2 or N < 2 or N > abi.QS_MAX_AGENTS or not 1 <= w.shape[1] <= N - 1 or w.shape[0] % N != 0 or w.shape[0] == 0 or tuple(ids.shape) != tuple(w.shape):
        raise ValueError(f"attention_matrix: weights and ids [E * {N}, K] with 1 <= K <= {N - 1} wanted, got {tuple(w.shape)} and {tuple(ids.shape)}")
    T, K = w.shape
    E = T // N
    if hasattr(w, "is_cuda") and w.is_cuda:
        import torch
        if w.dtype != torch.float32 or not (hasattr(ids, "is_cuda") and ids.is_cuda and ids.device == w.device and ids.dtype == torch.int32):
            raise ValueError("attention_matrix: device weights must be float32 and their ids an int32 tensor on the same device")
        w, ids = w.contiguous(), ids.contiguous()
        out = torch.empty((E, N, N), device=w.device, dtype=torch.float32)
        with torch.cuda.device(w.device):
            rc = native.lib().qs_neighbor_scatter(ids.data_ptr(), w.data_ptr(), E, N, K, out.data_ptr(), C.c_void_p(torch.cuda.current_stream(w.device).cuda_stream))
        if rc != 0:
            raise native.QsError(f"qs_neighbor_scatter failed ({rc}): {native.lib().qs_last_error().decode()}")
        return out
    is_tensor = hasattr(w, "new_zeros")
    wn, idn = (w.detach().numpy(), ids.detach().numpy() if hasattr(ids, "detach") else np.asarray(ids)) if is_tensor else (np.asarray(w), np.asarray(ids))
    out = np.zeros((E, N, N), dtype=wn.dtype)
    for g in range(T):
        e, i = divmod(g, N)
        for s in range(K):
            j = int(idn[g, s])
            if 0 <= j < N and j != i:
                out[e, i, j] = wn[g, s]
    if is_tensor:
        import torch
        return torch.from_numpy(out)
    return out
