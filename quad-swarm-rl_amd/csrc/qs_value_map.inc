// qs_value_map.inc - critic value maps over a grid of position offsets (include/quadswarm_valuemap.h: the semantics are stated THERE, once;
// part of qs_policy_encoder.hip's translation unit, behind its C ABI, because the middle of the sequence is qs_enc_forward).
//
//   expand   obs[A, D] -> rows[n, D]: row r = (agent a, cell i, cell j) is a's row with off_x[i] / off_y[j] added to the shifted columns
//   encoder  qs_enc_forward with a one-row head on the rows, chunk by chunk: values[r]
//   reduce   values[A, nx * ny] -> vmax, vmin, argmax per agent
//
// expand is a pure write stream (nx * ny * D * 4 bytes out per D * 4 bytes in; the source row of an agent is read nx * ny times and is meant
// to hit in L2 - nothing is staged).  Workgroup = 256 threads on ONE agent (blockIdx.x) and VM_UNROLL * 256 consecutive elements of that
// agent's nx * ny * D block (blockIdx.y); an element is a 16-byte quad of columns when D % 4 == 0 and both pointers are 16-byte aligned, one
// float otherwise - consecutive lanes write consecutive addresses, rows are dense, so a wave's store is 1 KiB (256 B) contiguous.  The offset
// tables and the shift list arrive in the launch arguments; every workgroup unpacks them once into LDS (one code byte per column: 0 = copy,
// 1 + axis + 2 * negative) and a thread looks its columns up there: no global table lookup per element, and an unshifted quad costs one
// 4-byte LDS read.  sign * off is a sign flip, so the shifted element is the ONE float32 add of the header.
// A chunk that begins or ends inside an agent's grid launches that agent's workgroups whole; the threads outside [row0, row0 + n) store nothing.
//
// reduce: one wave per agent (four to a workgroup), lane l takes elements l, l + 64, ... in rising order, then a butterfly of five
// __shfl_xor steps.  "Better" is a total order on (value, index) pairs - larger value, then smaller index; a NaN beats every number, and the
// earlier NaN the later - so the butterfly's result does not depend on the pairing and every lane ends with the same pair: fixed, atomic-free.

#include "../../include/quadswarm_valuemap.h"

#define VM_UNROLL 4

struct VmapExpandArgs {
    const float *obs;
    float *rows;
    long long row0;                       // first global row of this launch; rows[0] is that row
    int n_rows, D, nx, ny, a0, n_shifts;  // a0: agent of blockIdx.x == 0
    float off_x[QS_VMAP_MAX_GRID], off_y[QS_VMAP_MAX_GRID];
    uint32_t shift[QS_VMAP_MAX_SHIFTS];   // column | code << 16
};

__device__ __forceinline__ float vmap_shifted(float x, uint32_t code, const float (*s_off)[QS_VMAP_MAX_GRID], int i, int j) {
    if (code == 0) return x;
    const uint32_t c = code - 1;
    const float o = (c & 1) ? s_off[1][j] : s_off[0][i];
    return x + ((c & 2) ? -o : o);
}

template <int V>   // columns per element: 4 (one f32x4 per thread) or 1
__global__ void __launch_bounds__(256) qs_vmap_expand_kernel(const VmapExpandArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t s_code[QS_VMAP_MAX_OBS_DIM];
    __shared__ float s_off[2][QS_VMAP_MAX_GRID];
    const int tid = threadIdx.x, D = p.D;
    for (int c = tid * 4; c < D; c += 1024) *(uint32_t *)&s_code[c] = 0u;   // (D <= 4096 and the array is 4096: a word never passes its end)
    if (tid < QS_VMAP_MAX_GRID) s_off[0][tid] = p.off_x[tid];
    else if (tid < 2 * QS_VMAP_MAX_GRID) s_off[1][tid - QS_VMAP_MAX_GRID] = p.off_y[tid - QS_VMAP_MAX_GRID];
    __syncthreads();
    if (tid < p.n_shifts) { const uint32_t s = p.shift[tid]; s_code[s & 0xffffu] = (uint8_t)(s >> 16); }   // columns are distinct (validated)
    __syncthreads();

    const int DV = D / V, cells = p.nx * p.ny, per_agent = cells * DV;
    const int a = p.a0 + blockIdx.x;
    const float *__restrict__ src = p.obs + (size_t)a * D;
    const long long first = (long long)a * cells - p.row0;       // local row of this agent's cell 0 (negative: the chunk begins inside the grid)
#pragma unroll
    for (int u = 0; u < VM_UNROLL; ++u) {
        const int e = (blockIdx.y * VM_UNROLL + u) * 256 + tid;
        if (e >= per_agent) break;
        const int cell = e / DV, v = e - cell * DV;
        const long long rl = first + cell;
        if (rl < 0 || rl >= p.n_rows) continue;
        const int i = cell / p.ny, j = cell - i * p.ny;
        if constexpr (V == 4) {
            f32x4 x = ((const f32x4 *)src)[v];
            const uint32_t codes = *(const uint32_t *)&s_code[4 * v];
            if (codes != 0u) {
                x[0] = vmap_shifted(x[0], codes & 0xffu, s_off, i, j);
                x[1] = vmap_shifted(x[1], (codes >> 8) & 0xffu, s_off, i, j);
                x[2] = vmap_shifted(x[2], (codes >> 16) & 0xffu, s_off, i, j);
                x[3] = vmap_shifted(x[3], codes >> 24, s_off, i, j);
            }
            ((f32x4 *)(p.rows + (size_t)rl * D))[v] = x;
        } else {
            p.rows[(size_t)rl * D + v] = vmap_shifted(src[v], s_code[v], s_off, i, j);
        }
    }
}

// (value, index) x better than (value, index) b for the maximum (MAX) or the minimum: see the head of the file
template <bool MAX>
__device__ __forceinline__ bool vmap_better(float x, int xi, float b, int bi) {
    const bool xn = x != x, bn = b != b;
    if (xn || bn) return xn && (!bn || xi < bi);
    return (MAX ? x > b : x < b) || (x == b && xi < bi);
}

__global__ void __launch_bounds__(256) qs_vmap_reduce_kernel(const float *__restrict__ values, int A, int n, float *__restrict__ vmax,
                                                             float *__restrict__ vmin, int32_t *__restrict__ argmax) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= A) return;                                           // wave-uniform: the shuffles below run with all 64 lanes
    const float *__restrict__ v = values + (size_t)a * n;
    float hv = -__builtin_inff(), lv = __builtin_inff();          // lanes without an element hold (-inf / +inf, INT_MAX): worse than any element
    int hi = 0x7fffffff, li = 0x7fffffff;
    for (int k = lane; k < n; k += 64) {
        const float x = v[k];
        if (vmap_better<true>(x, k, hv, hi)) { hv = x; hi = k; }
        if (vmap_better<false>(x, k, lv, li)) { lv = x; li = k; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ohv = __shfl_xor(hv, m), olv = __shfl_xor(lv, m);
        const int ohi = __shfl_xor(hi, m), oli = __shfl_xor(li, m);
        if (vmap_better<true>(ohv, ohi, hv, hi)) { hv = ohv; hi = ohi; }
        if (vmap_better<false>(olv, oli, lv, li)) { lv = olv; li = oli; }
    }
    if (lane == 0) {
        if (vmax) vmax[a] = hv;
        if (vmin) vmin[a] = lv;
        if (argmax) argmax[a] = hi;
    }
}

static int vmap_fail(const char *fn, const char *what) { g_enc_error = std::string(fn) + ": " + what; return -1; }

// the grid (every entry point); 0 or -1
static int vmap_check_grid(const char *fn, const qs_value_map_params *p) {
    if (!p) return vmap_fail(fn, "NULL parameter struct");
    if (p->A < 1) return vmap_fail(fn, "A must be at least 1");
    if (p->nx < 1 || p->nx > QS_VMAP_MAX_GRID || p->ny < 1 || p->ny > QS_VMAP_MAX_GRID) return vmap_fail(fn, "nx and ny must be 1..64");
    return 0;
}

// what expand reads: rows, scratch, shift list; 0 or -1
static int vmap_check_expand(const char *fn, const qs_value_map_params *p) {
    if (vmap_check_grid(fn, p) != 0) return -1;
    if (!p->obs || !p->rows) return vmap_fail(fn, "obs and rows must not be NULL");
    if (p->obs_dim < 1 || p->obs_dim > QS_VMAP_MAX_OBS_DIM) return vmap_fail(fn, "obs_dim must be 1..4096");
    if (p->cap_rows < 1) return vmap_fail(fn, "cap_rows must be at least 1");
    if (p->n_shifts < 0 || p->n_shifts > QS_VMAP_MAX_SHIFTS) return vmap_fail(fn, "at most 64 shift entries");
    for (int s = 0; s < p->n_shifts; ++s) {
        if (p->shift_col[s] < 0 || p->shift_col[s] >= p->obs_dim) return vmap_fail(fn, "a shift column lies outside the row");
        if (p->shift_axis[s] != 0 && p->shift_axis[s] != 1) return vmap_fail(fn, "a shift axis must be 0 (x) or 1 (y)");
        if (p->shift_sign[s] != 1 && p->shift_sign[s] != -1) return vmap_fail(fn, "a shift sign must be +1 or -1");
        for (int t = 0; t < s; ++t)
            if (p->shift_col[t] == p->shift_col[s]) return vmap_fail(fn, "a shift column is named twice");
    }
    return 0;
}

static int vmap_launch_expand(const qs_value_map_params *p, int64_t row0, int32_t n_rows, hipStream_t stream) {
    VmapExpandArgs k;
    const int cells = p->nx * p->ny, D = p->obs_dim;
    k.obs = p->obs; k.rows = p->rows; k.row0 = row0; k.n_rows = n_rows; k.D = D; k.nx = p->nx; k.ny = p->ny; k.n_shifts = p->n_shifts;
    k.a0 = (int)(row0 / cells);
    for (int i = 0; i < QS_VMAP_MAX_GRID; ++i) { k.off_x[i] = i < p->nx ? p->off_x[i] : 0.0f; k.off_y[i] = i < p->ny ? p->off_y[i] : 0.0f; }
    for (int s = 0; s < QS_VMAP_MAX_SHIFTS; ++s)
        k.shift[s] = s < p->n_shifts ? (uint32_t)p->shift_col[s] | (uint32_t)(1 + p->shift_axis[s] + (p->shift_sign[s] < 0 ? 2 : 0)) << 16 : 0u;
    const int agents = (int)((row0 + n_rows - 1) / cells) - k.a0 + 1;
    const bool vec = D % 4 == 0 && (((size_t)p->obs | (size_t)p->rows) & 15) == 0;
    const int per_agent = cells * (vec ? D / 4 : D), per_block = 256 * VM_UNROLL;
    const dim3 grid(agents, (per_agent + per_block - 1) / per_block);
    if (vec) hipLaunchKernelGGL(qs_vmap_expand_kernel<4>, grid, dim3(256), 0, stream, k);
    else hipLaunchKernelGGL(qs_vmap_expand_kernel<1>, grid, dim3(256), 0, stream, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_enc_error = std::string("qs_value_map (expand): ") + hipGetErrorString(e); return -2; }
    return 0;
}

static int vmap_launch_reduce(const qs_value_map_params *p, hipStream_t stream) {
    if (!p->vmax && !p->vmin && !p->argmax) return 0;
    hipLaunchKernelGGL(qs_vmap_reduce_kernel, dim3((p->A + 3) / 4), dim3(256), 0, stream, (const float *)p->values, p->A, p->nx * p->ny,
                       p->vmax, p->vmin, p->argmax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_enc_error = std::string("qs_value_map (reduce): ") + hipGetErrorString(e); return -2; }
    return 0;
}

extern "C" {

size_t qs_value_map_sizeof_params(void) { return sizeof(qs_value_map_params); }

int qs_value_map_expand(const qs_value_map_params *p, int64_t row0, int32_t n_rows, void *stream) {
    const char *fn = "qs_value_map_expand";
    if (vmap_check_expand(fn, p) != 0) return -1;
    if (row0 < 0 || n_rows < 1 || n_rows > p->cap_rows || row0 + n_rows > (int64_t)p->A * p->nx * p->ny)
        return vmap_fail(fn, "rows row0 .. row0 + n_rows must lie inside the map and fit cap_rows");
    return vmap_launch_expand(p, row0, n_rows, (hipStream_t)stream);
}

int qs_value_map_reduce(const qs_value_map_params *p, void *stream) {
    const char *fn = "qs_value_map_reduce";
    if (vmap_check_grid(fn, p) != 0) return -1;
    if (!p->values) return vmap_fail(fn, "values must not be NULL");
    return vmap_launch_reduce(p, (hipStream_t)stream);
}

int qs_value_map(const qs_value_map_params *p, const qs_enc_params *critic, void *stream) {
    const char *fn = "qs_value_map";
    if (vmap_check_expand(fn, p) != 0) return -1;
    if (!p->values) return vmap_fail(fn, "values must not be NULL");
    if (!critic) return vmap_fail(fn, "NULL critic parameters");
    if (critic->head_dim != 1 || !critic->head_w || !critic->head_b) return vmap_fail(fn, "the critic needs a head of one row (head_dim == 1, head_w, head_b)");
    if (critic->obs_dim != p->obs_dim) return vmap_fail(fn, "critic obs_dim differs from the rows' obs_dim");
    qs_enc_params enc = *critic;
    enc.sample_log_std = nullptr; enc.act_out = nullptr; enc.sample_counter = nullptr;
    enc.traj_rew_src = nullptr; enc.traj_rew_dst = nullptr; enc.traj_done_src = nullptr; enc.traj_done_dst = nullptr;
    const int64_t total = (int64_t)p->A * p->nx * p->ny;
    for (int64_t row0 = 0; row0 < total; row0 += p->cap_rows) {
        const int32_t n = (int32_t)(total - row0 < p->cap_rows ? total - row0 : p->cap_rows);
        int rc = vmap_launch_expand(p, row0, n, (hipStream_t)stream);
        if (rc != 0) return rc;
        enc.head_out = p->values + row0;
        rc = qs_enc_forward(p->rows, n, &enc, nullptr, stream);
        if (rc != 0) return rc;
    }
    return vmap_launch_reduce(p, (hipStream_t)stream);
}

}
