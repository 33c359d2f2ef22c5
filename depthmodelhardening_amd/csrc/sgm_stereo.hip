// K35 -- a semi-global stereo matcher in integers for the depth-hint candidates (gfx950): the matcher DESIGN.md section 3 (K35)
// states, modelled on the structure of OpenCV's StereoSGBM in its single-pass mode (x-Sobel prefilter + Birchfield-Tomasi cost,
// block sum, five aggregation paths, winner-takes-all with a uniqueness test, sub-pixel parabola, left-right check, speckle
// filter).  Nothing is claimed about equality with OpenCV; the yardstick is tests/sgm_ref.py, bit for bit.
//
// A "job" is one (item, distinct parameter set): C and S int16 [H][Wv][D] (Wv = W - D, d fastest) in the workspace.  The host
// packs as many jobs as the workspace holds (at most MAXJ) into one sequence of launches; the job table travels by value in the
// kernel arguments, so nothing is uploaded and the whole call can be captured in a graph.
//
//   sgm_cost_kernel     one workgroup per TY x TX tile of matched pixels: the bytes of both views (mirrored reads for `reverse`),
//                       their prefiltered values and the lo / hi of both kinds for the tile's rows and columns with halo -> LDS;
//                       pc for the tile with halo -> LDS (int16); the (2r+1)^2 sum -> C.
//   sgm_path_kernel     one launch per direction.  A path is owned by a group of D / 4 lanes (rounded up to a power of two: 1, 2,
//                       4 ... paths per wave), four consecutive d per lane (one 8-byte load of C per step); the minimum over d is
//                       a butterfly inside the group, d - 1 / d + 1 come from the neighbouring slot or lane.  The two horizontal
//                       directions own a row each; the three from above own column (k + s y) mod Wv at row y, s = +1, 0, -1, and
//                       restart where they wrap (the path that left at the side ends, a new one starts at the border).  The first
//                       direction stores S, the later ones load, add and store: every (p, d) has one owner per launch.
//   sgm_select_kernel   one workgroup per row: the same lane groups take the lowest d of minimal S, the uniqueness test and the
//                       sub-pixel value; disp2 is an LDS atomicMin on (minS << 16) | x, which the tie rule makes unique; after a
//                       barrier the left-right check and the (mirrored) int16 store into every output slot of the job.
//   speckle             union-find over the stored map with integer atomicMin on the labels: the start of its horizontal run as
//                       every pixel's first label (a prefix maximum per row), merge of the vertical links, flatten + count with
//                       integer atomicAdd, mask.  Components are equivalence classes, so the result is unique.
// Integers only, no float, no host read.
#include "common.hpp"

#include <algorithm>

using namespace dmh;

namespace {

constexpr int MAXJ = 32;            // jobs per sequence of launches (the table is a kernel argument: 32 x 72 bytes)
constexpr int TY = 4, TX = 16, NT = 256;
constexpr int MAXW = DMH_SGM_MAX_WIDTH;
constexpr int BIG = 1 << 28;
constexpr int PC_MAX = 567;         // 3 (126 + 63)

struct Job {
    long long c_off, s_off, lab_off;    // byte offsets into the workspace
    int b, D, r, P1, P2, cap, uniq, d12, spw, sprange;
    unsigned out_mask;                  // the output slots n that receive this job's map
    int first;                          // the lowest of them: the speckle filter's working copy
};

struct Pack {
    int n, H, W, N;
    Job j[MAXJ];
};
static_assert(sizeof(Pack) <= 3072, "the job table must fit the kernel arguments");

__host__ __device__ inline long long align256(long long v) { return (v + 255) & ~255ll; }

// ---------------------------------------------------------------------------------------------------------------- cost
__host__ __device__ inline int cost_lds_bytes(int D, int r) {
    const int R = TY + 2 * r, CX = TX + 2 * r;
    const int entries = R * 6 * ((CX + 2) + (CX + D + 1));      // a byte (the value) and a word (value, lo, hi) each
    return ((entries + 3) & ~3) + 4 * entries + R * CX * D * 2;
}

__device__ __forceinline__ int bt_cost(int u, int lo_u, int hi_u, int v, int lo_v, int hi_v) {
    return min(max(0, max(u - hi_v, lo_v - u)), max(0, max(v - hi_u, lo_u - v)));
}

__global__ __launch_bounds__(NT) void sgm_cost_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ lookup,
                                                      const int32_t* __restrict__ reverse, const Pack pk, char* __restrict__ ws) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Job& jb = pk.j[blockIdx.z];
    const int H = pk.H, W = pk.W, D = jb.D, r = jb.r, Wv = W - D;
    const int xt0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    if (Wv <= 0 || xt0 >= Wv || y0 >= H) return;
    const int x0 = D + xt0;
    const int R = TY + 2 * r, CX = TX + 2 * r;
    const int wb = CX + 2, wl = CX + D + 1;         // staged columns of the base and of the lookup view
    const int ob = x0 - r - 1, ol = x0 - r - D;     // their first columns (may lie outside the image: replicated)
    const int wsum = wb + wl;
    unsigned char* s_val = smem;                    // [R][6][wsum]: base columns, then lookup columns; kinds g0 g1 g2 I0 I1 I2
    unsigned* s_vlh = (unsigned*)(smem + ((R * 6 * wsum + 3) & ~3));       // the same entries as value | lo << 8 | hi << 16
    int16_t* s_pc = (int16_t*)(s_vlh + R * 6 * wsum);                      // [R][CX][D]
    const bool rev = reverse != nullptr && reverse[jb.b] != 0;
    const int64_t plane = (int64_t)H * W;
    const int tid = threadIdx.x, cap = jb.cap;

    for (int e = tid; e < R * wsum; e += NT) {
        const int ry = e / wsum, i = e % wsum;
        const bool is_l = i >= wb;
        const int col = min(max(is_l ? ol + (i - wb) : ob + i, 0), W - 1);
        const int y = min(max(y0 - r + ry, 0), H - 1), yu = max(y - 1, 0), yd = min(y + 1, H - 1);
        const uint8_t* img = (is_l ? lookup : base) + (int64_t)jb.b * 3 * plane;
        const int cm = max(col - 1, 0), cp = min(col + 1, W - 1);
        const int mc = rev ? W - 1 - col : col, mm = rev ? W - 1 - cm : cm, mp = rev ? W - 1 - cp : cp;
        const bool edge = col == 0 || col == W - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* p = img + c * plane;
            const int s = ((int)p[(int64_t)yu * W + mp] - (int)p[(int64_t)yu * W + mm])
                          + 2 * ((int)p[(int64_t)y * W + mp] - (int)p[(int64_t)y * W + mm])
                          + ((int)p[(int64_t)yd * W + mp] - (int)p[(int64_t)yd * W + mm]);
            s_val[(ry * 6 + c) * wsum + i] = (unsigned char)(edge ? cap : min(max(s, -cap), cap) + cap);
            s_val[(ry * 6 + 3 + c) * wsum + i] = p[(int64_t)y * W + mc];
        }
    }
    __syncthreads();
    for (int e = tid; e < R * 6 * wsum; e += NT) {
        const int i = e % wsum;
        // the first and last staged column of either view have no staged neighbour, and are never read
        const int im = (i == 0 || i == wb) ? i : i - 1, ip = (i == wb - 1 || i == wsum - 1) ? i : i + 1;
        const int a = s_val[e], l = s_val[e - i + im], rr = s_val[e - i + ip];
        const int hl = (a + l) >> 1, hr = (a + rr) >> 1;
        s_vlh[e] = (unsigned)a | ((unsigned)min(a, min(hl, hr)) << 8) | ((unsigned)max(a, max(hl, hr)) << 16);
    }
    __syncthreads();
    // a wave per staged pixel, the lanes across d: the base view's six words are wave-uniform, the lookup view's consecutive
    const int wave = tid / WAVE, lane = tid & (WAVE - 1);
    for (int p = wave; p < R * CX; p += NT / WAVE) {
        const int rx = p % CX, ry = p / CX;
        const int xc = min(max(x0 - r + rx, D), W - 1);
        const int ib = xc - ob, il = wb + (xc - ol);
        unsigned u[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) u[k] = s_vlh[(ry * 6 + k) * wsum + ib];
        for (int d = lane; d < D; d += WAVE) {
            int acc = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const unsigned v = s_vlh[(ry * 6 + k) * wsum + il - d];
                const int t = bt_cost(u[k] & 255, (u[k] >> 8) & 255, u[k] >> 16, v & 255, (v >> 8) & 255, v >> 16);
                acc += k < 3 ? t : (t >> 2);
            }
            s_pc[p * D + d] = (int16_t)acc;
        }
    }
    __syncthreads();
    int16_t* C = (int16_t*)(ws + jb.c_off);
    for (int p = wave; p < TY * TX; p += NT / WAVE) {
        const int tx = p % TX, ty = p / TX;
        const int y = y0 + ty, xi = xt0 + tx;
        if (y >= H || xi >= Wv) continue;
        for (int d = lane; d < D; d += WAVE) {
            int acc = 0;
            for (int dy = 0; dy <= 2 * r; ++dy)
                for (int dx = 0; dx <= 2 * r; ++dx) acc += s_pc[((ty + dy) * CX + tx + dx) * D + d];
            C[((int64_t)y * Wv + xi) * D + d] = (int16_t)acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- lane groups
// D / 4 lanes own one pixel's D values, four consecutive d per lane; GW is that count rounded up to a power of two.
struct Group {
    int G, GW, per_wave, g, slot;       // lanes in use, group width, groups per wave, this lane's place in its group, its group
    bool live;                          // this lane holds four d < D
};

__device__ __forceinline__ Group make_group(int D) {
    Group q;
    q.G = D >> 2;
    int gw = 4;
    while (gw < q.G) gw <<= 1;
    q.GW = gw;
    q.per_wave = WAVE / gw;
    const int lane = threadIdx.x & (WAVE - 1);
    q.g = lane & (gw - 1);
    q.slot = lane / gw;
    q.live = q.g < q.G;
    return q;
}

__device__ __forceinline__ int group_min(int v, int GW) {
    for (int o = GW >> 1; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, WAVE));
    return v;
}

__device__ __forceinline__ void unpack4(uint2 w, int v[4]) {
    v[0] = (int)(int16_t)(w.x & 0xffffu);
    v[1] = (int)(int16_t)(w.x >> 16);
    v[2] = (int)(int16_t)(w.y & 0xffffu);
    v[3] = (int)(int16_t)(w.y >> 16);
}

__device__ __forceinline__ uint2 pack4(const int v[4]) {
    return make_uint2(((unsigned)v[0] & 0xffffu) | ((unsigned)v[1] << 16), ((unsigned)v[2] & 0xffffu) | ((unsigned)v[3] << 16));
}

// ---------------------------------------------------------------------------------------------------------------- paths
// dir: 0 from (x-1, y), 1 from (x+1, y), 2 from (x-1, y-1), 3 from (x, y-1), 4 from (x+1, y-1)
__global__ __launch_bounds__(NT) void sgm_path_kernel(const Pack pk, char* __restrict__ ws, int dir, int first) {
    const Job& jb = pk.j[blockIdx.y];
    const int H = pk.H, D = jb.D, Wv = pk.W - D;
    if (Wv <= 0) return;
    const Group q = make_group(D);
    const int npaths = dir < 2 ? H : Wv, nsteps = dir < 2 ? Wv : H;
    const int path = (blockIdx.x * (NT / WAVE) + threadIdx.x / WAVE) * q.per_wave + q.slot;
    // a wave whose first path is past the end has nothing to do; inside a wave every lane keeps taking part in the shuffles
    if ((blockIdx.x * (NT / WAVE) + threadIdx.x / WAVE) * q.per_wave >= npaths) return;
    const bool act = q.live && path < npaths;
    const uint2* C = (const uint2*)(ws + jb.c_off);
    uint2* S = (uint2*)(ws + jb.s_off);
    const int P1 = jb.P1, P2 = jb.P2, wordsD = D >> 2;

    int x = dir < 2 ? (dir == 0 ? 0 : Wv - 1) : (path < npaths ? path : 0), y = dir < 2 ? (path < npaths ? path : 0) : 0;
    int Lp[4] = {BIG, BIG, BIG, BIG};
    int64_t o = ((int64_t)y * Wv + x) * wordsD + q.g;
    uint2 cw = act ? C[o] : make_uint2(0, 0), sw = (act && !first) ? S[o] : make_uint2(0, 0);
    for (int t = 0; t < nsteps; ++t) {
        const bool reset = t == 0 || (dir == 2 && x == 0) || (dir == 4 && x == Wv - 1);
        // where the next step is, and its loads (they do not depend on the recurrence)
        int nx = x, ny = y;
        if (dir == 0) nx = x + 1;
        else if (dir == 1) nx = x - 1;
        else {
            ny = y + 1;
            if (dir == 2) nx = x + 1 == Wv ? 0 : x + 1;
            if (dir == 4) nx = x == 0 ? Wv - 1 : x - 1;
        }
        const int64_t no = ((int64_t)ny * Wv + nx) * wordsD + q.g;
        const bool more = act && t + 1 < nsteps;
        const uint2 ncw = more ? C[no] : make_uint2(0, 0), nsw = (more && !first) ? S[no] : make_uint2(0, 0);

        int c[4], L[4];
        unpack4(cw, c);
        int m = min(min(Lp[0], Lp[1]), min(Lp[2], Lp[3]));
        m = group_min(m, q.GW);
        int below = __shfl_up(Lp[3], 1, WAVE), above = __shfl_down(Lp[0], 1, WAVE);
        if (q.g == 0) below = BIG;
        if (q.g >= q.G - 1) above = BIG;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dm = k == 0 ? below : Lp[k - 1], dp = k == 3 ? above : Lp[k + 1];
            const int best = min(min(Lp[k], min(dm, dp) + P1), m + P2) - m;
            L[k] = !act ? BIG : (reset ? c[k] : c[k] + best);
        }
        if (act) {
            if (first) S[o] = pack4(L);
            else {
                int s[4];
                unpack4(sw, s);
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] += L[k];
                S[o] = pack4(s);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) Lp[k] = L[k];
        x = nx;
        y = ny;
        o = no;
        cw = ncw;
        sw = nsw;
    }
}

// ---------------------------------------------------------------------------------------------------------------- select
__global__ __launch_bounds__(NT) void sgm_select_kernel(const int32_t* __restrict__ reverse, const Pack pk, const char* __restrict__ ws,
                                                        int16_t* __restrict__ out) {
    __shared__ unsigned s_key[MAXW];
    __shared__ int16_t s_value[MAXW];
    __shared__ uint8_t s_dstar[MAXW];
    const Job& jb = pk.j[blockIdx.y];
    const int H = pk.H, W = pk.W, D = jb.D, Wv = W - D, y = blockIdx.x, tid = threadIdx.x;
    for (int x = tid; x < W; x += NT) {
        s_key[x] = 0xffffffffu;
        s_value[x] = -16;
        s_dstar[x] = 0;
    }
    __syncthreads();
    if (Wv > 0) {
        const Group q = make_group(D);
        const uint2* S = (const uint2*)(ws + jb.s_off);
        const int16_t* S16 = (const int16_t*)(ws + jb.s_off);
        const int per_block = (NT / WAVE) * q.per_wave, mine = (tid / WAVE) * q.per_wave + q.slot;
        const int wordsD = D >> 2, keep = 100 - jb.uniq;
        for (int x0 = 0; x0 < Wv; x0 += per_block) {          // uniform trip count: every lane takes part in the shuffles
            const int xi = x0 + mine;
            const bool act = q.live && xi < Wv;
            const int64_t row = ((int64_t)y * Wv + (xi < Wv ? xi : 0));
            int s[4] = {BIG, BIG, BIG, BIG};
            if (act) unpack4(S[row * wordsD + q.g], s);
            int key = BIG;
#pragma unroll
            for (int k = 0; k < 4; ++k) key = min(key, act ? (s[k] << 8) | (q.g * 4 + k) : BIG);
            key = group_min(key, q.GW);                      // the lowest S, the lowest d among equals
            const int min_s = key >> 8, d_star = key & 255;
            int dropped = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = q.g * 4 + k, gap = d > d_star ? d - d_star : d_star - d;
                if (act && gap > 1 && s[k] * keep < 100 * min_s) dropped = 1;
            }
            dropped = -group_min(-dropped, q.GW);
            if (act && q.g == 0 && !dropped) {
                const int x = xi + D;
                int v = 16 * d_star;
                if (d_star > 0 && d_star < D - 1) {
                    const int sm = S16[row * D + d_star - 1], sp = S16[row * D + d_star + 1];
                    const int den = max(sm + sp - 2 * min_s, 1);
                    v += ((sm - sp) * 16 + den) / (2 * den);
                }
                s_value[x] = (int16_t)v;
                s_dstar[x] = (uint8_t)d_star;
                atomicMin(&s_key[x - d_star], ((unsigned)min_s << 16) | (unsigned)x);
            }
        }
    }
    __syncthreads();
    const bool rev = reverse != nullptr && reverse[jb.b] != 0;
    for (int x = tid; x < W; x += NT) {
        int v = s_value[x];
        if (v >= 0) {
            int bad = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int dd = (v + 15 * k) >> 4, x2 = x - dd;
                if (x2 >= 0 && x2 < W) {
                    const unsigned key = s_key[x2];
                    if (key != 0xffffffffu) {
                        const int d2 = s_dstar[key & 0xffffu];
                        bad += (d2 > dd ? d2 - dd : dd - d2) > jb.d12;
                    }
                }
            }
            if (bad == 2) v = -16;
        }
        const int xo = rev ? W - 1 - x : x;
        for (unsigned mask = jb.out_mask, n = 0; mask != 0; mask >>= 1, ++n)
            if (mask & 1u) out[(((int64_t)jb.b * pk.N + n) * H + y) * W + xo] = (int16_t)v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- speckle
__device__ __forceinline__ int find_root(int* lab, int i) {
    int p;
    while ((p = __atomic_load_n(&lab[i], __ATOMIC_RELAXED)) != i) i = p;
    return i;
}

__device__ __forceinline__ void unite(int* lab, int a, int b) {
    while (true) {
        a = find_root(lab, a);
        b = find_root(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&lab[a], b);      // the larger root points at the smaller one, unless somebody moved it first
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ bool speckle_linked(int a, int b, int range) { return a >= 0 && b >= 0 && (a > b ? a - b : b - a) <= range; }

// The first labels: one workgroup per row takes every valid pixel to the start of its horizontal run (a prefix maximum over the
// columns where a run starts) and counts the run's length at its start, so that the merge pass has only the vertical links left
// and no chain is longer than two hops before it.  Labelling every pixel with itself and uniting all neighbours gives the same components through chains as long as a
// run: 51 ms of speckle filter for 8 pairs of 320 x 1024 (has the present time).
__global__ __launch_bounds__(NT) void sgm_speckle_rows_kernel(const Pack pk, char* __restrict__ ws, const int16_t* __restrict__ out) {
    __shared__ int s_scan[NT];
    __shared__ int s_start[NT + 1];
    __shared__ int s_carry;
    const Job& jb = pk.j[blockIdx.y];
    if (jb.spw <= 0) return;
    const int H = pk.H, W = pk.W, y = blockIdx.x, tid = threadIdx.x;
    int* lab = (int*)(ws + jb.lab_off);
    int* size = lab + H * W;
    const int16_t* row = out + (((int64_t)jb.b * pk.N + jb.first) * H + y) * W;
    for (int x = tid; x < W; x += NT) size[y * W + x] = 0;
    if (tid == 0) {
        s_carry = 0;
        s_start[NT] = 0;        // the pixel after a chunk's last one: a run's part ends with the chunk
    }
    __syncthreads();
    for (int x0 = 0; x0 < W; x0 += NT) {
        const int x = x0 + tid;
        int v = -16, start = -1;
        if (x < W) {
            v = row[x];
            if (x == 0 || !speckle_linked(v, row[x - 1], jb.sprange)) start = x;        // an invalid pixel breaks the run too
        } else {
            start = x;
        }
        s_scan[tid] = start;
        s_start[tid] = start;
        __syncthreads();
        for (int o = 1; o < NT; o <<= 1) {
            const int t = tid >= o ? s_scan[tid - o] : -1;
            __syncthreads();
            s_scan[tid] = max(s_scan[tid], t);
            __syncthreads();
        }
        const int run = s_scan[tid] >= 0 ? s_scan[tid] : s_carry;
        if (x < W) {
            lab[y * W + x] = v >= 0 ? y * W + run : -1;
            // the length of a run is counted at its start, one addition per chunk it crosses (all by this workgroup)
            if (v >= 0 && s_start[tid + 1] >= 0) atomicAdd(&size[y * W + run], x - max(run, x0) + 1);
        }
        __syncthreads();
        if (tid == NT - 1) s_carry = run;
        __syncthreads();
    }
}

// phase 1 merge (the vertical links), 2 flatten + count, 3 mask
__global__ __launch_bounds__(NT) void sgm_speckle_kernel(const Pack pk, char* __restrict__ ws, int16_t* __restrict__ out, int phase) {
    const Job& jb = pk.j[blockIdx.y];
    if (jb.spw <= 0) return;
    const int H = pk.H, W = pk.W, total = H * W;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    int* lab = (int*)(ws + jb.lab_off);
    int* size = lab + total;
    const int16_t* map = out + ((int64_t)jb.b * pk.N + jb.first) * total;
    const int v = map[i];
    if (phase == 1) {
        if (v < 0 || i + W >= total) return;
        const int below = map[i + W];
        if (!speckle_linked(v, below, jb.sprange)) return;
        if (i % W > 0) {
            // the left neighbours are in the same two runs and linked to each other: their link already unites the runs
            const int left = map[i - 1], left_below = map[i + W - 1];
            if (speckle_linked(v, left, jb.sprange) && speckle_linked(below, left_below, jb.sprange)
                && speckle_linked(left, left_below, jb.sprange)) return;
        }
        unite(lab, i, i + W);
    } else if (phase == 2) {
        if (v < 0) return;
        const int root = find_root(lab, i);
        __atomic_store_n(&lab[i], root, __ATOMIC_RELAXED);      // only ever shortens a chain that ends at root
        // a run that is not its component's root hands its length over: one addition per run, not per pixel (a component of
        // 280,000 pixels made as many additions to one address).  size[i] of such a run is final since the rows pass.
        const bool starts = i % W == 0 || !speckle_linked(v, map[i - 1], jb.sprange);
        if (starts && root != i) atomicAdd(&size[root], size[i]);
    } else {
        int w = v;
        if (v >= 0 && size[find_root(lab, i)] <= jb.spw) w = -16;
        for (unsigned mask = jb.out_mask, n = 0; mask != 0; mask >>= 1, ++n)
            if (mask & 1u) out[((int64_t)jb.b * pk.N + n) * total + i] = (int16_t)w;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct Unique {
    dmh_sgm_params p;
    int r;
    unsigned mask;
    int first;
};

int check_params(const char* fn, const dmh_sgm_params* params, int N) {
#define SGM_REQUIRE(cond, msg)                                                              \
    do {                                                                                    \
        if (!(cond)) return dmh::fail(DMH_EINVAL, "%s: requirement failed: " msg, fn);      \
    } while (0)
    SGM_REQUIRE(params != nullptr, "null pointer");
    SGM_REQUIRE(N >= 1 && N <= DMH_SGM_MAX_MATCHERS, "need 1 <= N <= 16 parameter sets");
    for (int n = 0; n < N; ++n) {
        const dmh_sgm_params& p = params[n];
        SGM_REQUIRE(p.min_disparity == 0, "minDisparity must be 0");
        SGM_REQUIRE(p.num_disparities >= 16 && p.num_disparities <= 256 && p.num_disparities % 16 == 0,
                    "numDisparities must be a multiple of 16 in [16, 256]");
        SGM_REQUIRE(p.block_size >= 1 && p.block_size <= 3, "blockSize must be 1, 2 or 3 (radius <= 1: int16 sums are exact)");
        SGM_REQUIRE(p.P1 >= 0 && p.P2 >= 0, "P1 and P2 must not be negative");
        const int side = 2 * (p.block_size / 2) + 1;
        SGM_REQUIRE(p.P2 <= 32767 && 5 * (side * side * PC_MAX + p.P2) < 32767, "5 ((2r+1)^2 567 + P2) must stay below 32767 (int16 sums)");
        SGM_REQUIRE(p.pre_filter_cap >= 1 && p.pre_filter_cap <= 63, "preFilterCap must lie in [1, 63]");
        SGM_REQUIRE(p.uniqueness_ratio >= 0 && p.uniqueness_ratio <= 100, "uniquenessRatio must lie in [0, 100]");
        SGM_REQUIRE(p.disp12_max_diff >= 0 && p.disp12_max_diff <= 32767, "disp12MaxDiff must lie in [0, 32767]");
        SGM_REQUIRE(p.speckle_window_size >= 0, "speckleWindowSize must not be negative");
        SGM_REQUIRE(p.speckle_range >= 0 && p.speckle_range <= 4096, "speckleRange must lie in [0, 4096]");
    }
#undef SGM_REQUIRE
    return DMH_OK;
}

int check_shape(const char* fn, int B, int H, int W, int N) {
    if (!(B >= 1 && H >= 1 && W >= 1)) return dmh::fail(DMH_EINVAL, "%s: requirement failed: need B, H, W >= 1", fn);
    if (!(W <= MAXW && H <= 65535))
        return dmh::fail(DMH_EINVAL, "%s: requirement failed: need W <= 4096 (a row's disp2 lives in LDS) and H <= 65535", fn);
    if (!((int64_t)B * N * H * W < (1ll << 31) && (int64_t)B * 3 * H * W < (1ll << 31)))
        return dmh::fail(DMH_EINVAL, "%s: requirement failed: B N H W and B 3 H W must stay below 2^31", fn);
    return DMH_OK;
}

// the distinct jobs of a parameter list: blockSize enters through its radius only
int distinct(const dmh_sgm_params* params, int N, Unique* u) {
    int nu = 0;
    for (int n = 0; n < N; ++n) {
        dmh_sgm_params p = params[n];
        const int r = p.block_size / 2;
        p.block_size = 2 * r + 1;
        int k = 0;
        for (; k < nu; ++k)
            if (memcmp(&u[k].p, &p, sizeof(p)) == 0) break;
        if (k == nu) {
            u[nu].p = p;
            u[nu].r = r;
            u[nu].mask = 0;
            u[nu].first = n;
            ++nu;
        }
        u[k].mask |= 1u << n;
    }
    return nu;
}

struct JobBytes {
    long long c, lab;
};

JobBytes job_bytes(const Unique& u, int H, int W) {
    const int Wv = W - u.p.num_disparities;
    JobBytes jb;
    jb.c = Wv > 0 ? align256(2ll * H * Wv * u.p.num_disparities) : 0;
    jb.lab = u.p.speckle_window_size > 0 ? align256(8ll * H * W) : 0;
    return jb;
}

// Greedy packing of the jobs (item-major) under `limit` bytes and MAXJ jobs.  visit(pack) is called for every pack; returns the
// number of packs, or -1 when one job alone is over the limit.  *peak: the largest pack.
template <typename Visit>
int for_each_pack(int B, int H, int W, int N, const Unique* u, int nu, long long limit, long long* peak, Visit visit) {
    Pack pk;
    pk.H = H;
    pk.W = W;
    pk.N = N;
    pk.n = 0;
    long long used = 0;
    int packs = 0;
    *peak = 0;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nu; ++k) {
            const JobBytes jb = job_bytes(u[k], H, W);
            const long long need = 2 * jb.c + jb.lab;
            if (need > limit) return -1;
            if (pk.n == MAXJ || used + need > limit) {
                visit(pk);
                ++packs;
                pk.n = 0;
                used = 0;
            }
            Job& j = pk.j[pk.n++];
            j.c_off = used;
            j.s_off = used + jb.c;
            j.lab_off = used + 2 * jb.c;
            j.b = b;
            j.D = u[k].p.num_disparities;
            j.r = u[k].r;
            j.P1 = u[k].p.P1;
            j.P2 = u[k].p.P2;
            j.cap = u[k].p.pre_filter_cap;
            j.uniq = u[k].p.uniqueness_ratio;
            j.d12 = u[k].p.disp12_max_diff;
            j.spw = u[k].p.speckle_window_size;
            j.sprange = 16 * u[k].p.speckle_range;
            j.out_mask = u[k].mask;
            j.first = u[k].first;
            used += need;
            if (used > *peak) *peak = used;
        }
    if (pk.n > 0) {
        visit(pk);
        ++packs;
    }
    return packs;
}

std::atomic<uint64_t> g_cost_lds_done{0};

}  // namespace

extern "C" {

int64_t dmh_sgm_plan(int B, int H, int W, const dmh_sgm_params* params, int N, int64_t cap_bytes, int* n_chunks) {
    if (check_params("dmh_sgm_plan", params, N) != DMH_OK || check_shape("dmh_sgm_plan", B, H, W, N) != DMH_OK) return -1;
    if (cap_bytes < 1) {
        dmh::fail(DMH_EINVAL, "%s: requirement failed: the workspace cap must be positive", "dmh_sgm_plan");
        return -1;
    }
    Unique u[DMH_SGM_MAX_MATCHERS];
    const int nu = distinct(params, N, u);
    long long peak = 0;
    const int packs = for_each_pack(B, H, W, N, u, nu, cap_bytes, &peak, [](const Pack&) {});
    if (packs < 0) {
        dmh::fail(DMH_EINVAL, "%s: one matcher of one item needs more workspace than the cap allows", "dmh_sgm_plan");
        return -1;
    }
    if (n_chunks != nullptr) *n_chunks = packs;
    return peak > 256 ? peak : 256;
}

int dmh_sgm_disparity(const uint8_t* base, const uint8_t* lookup, const int32_t* reverse, int B, int H, int W,
                      const dmh_sgm_params* params, int N, int16_t* out, void* ws, int64_t ws_bytes, int phases, void* stream) {
    DMH_REQUIRE(base && lookup && out && ws, "null pointer");
    DMH_REQUIRE(phases >= 1 && phases <= DMH_SGM_ALL, "phases must be a non-empty subset of DMH_SGM_ALL");
    int rc = check_params("dmh_sgm_disparity", params, N);
    if (rc != DMH_OK) return rc;
    rc = check_shape("dmh_sgm_disparity", B, H, W, N);
    if (rc != DMH_OK) return rc;
    DMH_REQUIRE(((uintptr_t)out & 1) == 0 && ((uintptr_t)reverse & 3) == 0 && ((uintptr_t)ws & 255) == 0,
                "out must be 2-byte, reverse 4-byte and the workspace 256-byte aligned");
    DMH_REQUIRE((const void*)out != (const void*)base && (const void*)out != (const void*)lookup && (const void*)out != ws
                    && ws != (const void*)base && ws != (const void*)lookup, "out and the workspace must not alias the images or each other");
    DMH_REQUIRE(ws_bytes >= 256, "the workspace holds at least 256 bytes (dmh_sgm_plan)");
    Unique u[DMH_SGM_MAX_MATCHERS];
    const int nu = distinct(params, N, u);
    long long peak = 0;
    if (for_each_pack(B, H, W, N, u, nu, ws_bytes, &peak, [](const Pack&) {}) < 0)
        return dmh::fail(DMH_EINVAL, "%s: requirement failed: the workspace is smaller than one matcher of one item needs (dmh_sgm_plan)",
                         "dmh_sgm_disparity");
    int max_lds = 0;
    for (int k = 0; k < nu; ++k) max_lds = std::max(max_lds, cost_lds_bytes(u[k].p.num_disparities, u[k].r));
    if (max_lds > 48 * 1024) {
        // sized for the widest matcher the entry point takes, so that the attribute is set once per device
        const int widest = cost_lds_bytes(256, 1);
        if (configure_dynamic_lds(sgm_cost_kernel, (size_t)widest, g_cost_lds_done) != hipSuccess)
            return dmh::fail(DMH_ELAUNCH, "%s: cannot reserve the cost kernel's LDS", "dmh_sgm_disparity");
    }
    hipStream_t st = (hipStream_t)stream;
    char* wsp = (char*)ws;
    for_each_pack(B, H, W, N, u, nu, ws_bytes, &peak, [&](const Pack& pk) {
        int max_wv = 0, max_paths_blocks[2] = {0, 0}, lds = 0, any_speckle = 0;
        for (int i = 0; i < pk.n; ++i) {
            const Job& j = pk.j[i];
            const int Wv = W - j.D;
            if (j.spw > 0) any_speckle = 1;
            if (Wv <= 0) continue;
            max_wv = std::max(max_wv, Wv);
            lds = std::max(lds, cost_lds_bytes(j.D, j.r));
            int gw = 4;
            while (gw < j.D / 4) gw <<= 1;
            const int per_block = (NT / WAVE) * (WAVE / gw);
            max_paths_blocks[0] = std::max(max_paths_blocks[0], (H + per_block - 1) / per_block);
            max_paths_blocks[1] = std::max(max_paths_blocks[1], (Wv + per_block - 1) / per_block);
        }
        if (max_wv > 0 && (phases & DMH_SGM_COST))
            hipLaunchKernelGGL(sgm_cost_kernel, dim3((max_wv + TX - 1) / TX, (H + TY - 1) / TY, pk.n), dim3(NT), lds, st, base, lookup,
                               reverse, pk, wsp);
        if (max_wv > 0 && (phases & DMH_SGM_PATHS))
            for (int dir = 0; dir < 5; ++dir)
                hipLaunchKernelGGL(sgm_path_kernel, dim3(max_paths_blocks[dir < 2 ? 0 : 1], pk.n), dim3(NT), 0, st, pk, wsp, dir,
                                   dir == 0 ? 1 : 0);
        if (phases & DMH_SGM_SELECT)
            hipLaunchKernelGGL(sgm_select_kernel, dim3(H, pk.n), dim3(NT), 0, st, reverse, pk, (const char*)wsp, out);
        if (any_speckle && (phases & DMH_SGM_SPECKLE)) {
            hipLaunchKernelGGL(sgm_speckle_rows_kernel, dim3(H, pk.n), dim3(NT), 0, st, pk, wsp, (const int16_t*)out);
            for (int phase = 1; phase < 4; ++phase)
                hipLaunchKernelGGL(sgm_speckle_kernel, dim3((H * W + NT - 1) / NT, pk.n), dim3(NT), 0, st, pk, wsp, out, phase);
        }
    });
    return check_launch("dmh_sgm_disparity");
}

}  // extern "C"
