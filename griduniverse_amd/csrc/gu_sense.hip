// gu_sense.hip -- the agent's sensors: what every env of the batch SEES, as small uint8 views (include/gu.h: gu_sense).
//
// The reference ships no sensor (its roadmap asks for one: the field of view "constrained to the current state, surrounding
// states or the complete grid"); the rule is build-defined and stated in include/gu.h.  The class of a cell is the viewer's tile
// rule (gu_tile.hpp: gu_tile_kind, core/envs/rendering.py:119-133), 4 outside the grid.
//
// Store layout.  The output is dense, [rows][envs][V] bytes with V = K * K (GU_SENSE_EGO, K = 2r + 1) or H * W (GU_SENSE_GRID), and
// the kernel is write-dominated: V bytes per env-step against 4 read.  V is odd for every K, so no env's view starts on a 16-byte
// boundary and a lane that owned an env would store bytes.  Instead a lane owns an aligned 16-byte PIECE of the flat output and
// writes it with one vector store (a wave: 1 KiB contiguous); the sixteen bytes find their own (env-step, dy, dx): one division
// by the constants V and K per piece (the radius is a template argument), carries from there on.  The buffer is rounded up to 16
// bytes, the bytes past the end are computed like the others from the last env-step, and the host copy takes the real ones.
//
// Class plane.  A workgroup writes GU_SENSE_CHUNK contiguous bytes.  Where ONE grid serves all the env-steps of that chunk -- a
// single-grid engine, or a chunk inside one group of a multi-grid one -- and the plane fits GU_SENSE_LDS_BYTES, the workgroup stages
// the grid's class plane in LDS, padded by r cells of class 4 on every side (device mazes: flags turned into classes on the
// way), and the inner loop is one LDS byte read per output byte, no bounds test.  Otherwise (the chunk spans grids, e.g. one
// grid per env; or a large grid) every byte reads its class from global memory -- the planes are small and shared, L2 serves them
// -- behind the bounds test.  The choice is made per workgroup and is the same for all its lanes.
#include "gu_internal.hpp"
#include "gu_tile.hpp"

#define GU_SENSE_BLOCK 256
#define GU_SENSE_PIECES 4                                           /* 16-byte pieces per lane */
#define GU_SENSE_CHUNK (GU_SENSE_BLOCK * GU_SENSE_PIECES * 16)      /* bytes per workgroup: 16 KiB */
// The padded plane a workgroup may stage: half the bytes it writes (staging more than that per chunk costs more than the bounds
// tests it saves); 32 x 32 at r = 7 needs 2116, 64 x 64 at r = 7 6084, the whole-grid view of 90 x 90 8100.
#define GU_SENSE_LDS_BYTES 8192

struct SenseArgs {
    const uint8_t *cell;   // [G][flags | reward]
    const uint8_t *kind;   // [G][cell_bytes] class plane, or nullptr (device mazes: from the flags)
    const int32_t *src;    // position of env-step q: src[q * src_stride] (pos + env0; or the obs words of the first row asked for)
    uint8_t *out;          // [n_pieces * 16]
    int64_t n_steps;       // env-steps: rows * n
    int64_t n_pieces;      // ceil(n_steps * V / 16)
    int64_t env0, n;       // env of env-step q: env0 + q % n
    int64_t group, grid_stride, kind_stride;
    int32_t src_stride;    // 1 (pos, obs plane) or 3 (triples)
    int32_t W, H, S, n_grids;
};

// the class plane of grid g in LDS, padded by R cells of class 4 on every side
template <int R>
__device__ __forceinline__ void gu_sense_stage(const SenseArgs &a, int64_t g, uint8_t *plane)
{
    const uint8_t *flags = a.cell + g * a.grid_stride;
    const uint8_t *kind = a.kind ? a.kind + g * a.kind_stride : nullptr;
    const int32_t Wp = a.W + 2 * R, cells = Wp * (a.H + 2 * R);
    for (int32_t i = threadIdx.x; i < cells; i += GU_SENSE_BLOCK) {
        const int32_t y = i / Wp - R, x = i % Wp - R;
        uint32_t c = 4u;
        if ((uint32_t)y < (uint32_t)a.H && (uint32_t)x < (uint32_t)a.W) {
            const int32_t s = y * a.W + x;
            c = gu_tile_kind(kind, flags[s], s);
        }
        plane[i] = (uint8_t)c;
    }
    __syncthreads();
}

// Where a lane stands in the flat output: env-step q (clamped to the last one for the bytes past the end), its position, and what
// the byte's class is read from.
template <int R, bool GRID, bool LDS>
struct SenseCursor {
    const SenseArgs &a;
    const uint8_t *plane;  // LDS: the padded plane
    const uint8_t *flags = nullptr, *kind = nullptr;  // L2: the env's grid
    int64_t q, e = 0;
    int32_t p = 0, y = 0, x = 0, base = 0;

    __device__ __forceinline__ SenseCursor(const SenseArgs &args, const uint8_t *lds, int64_t q0) : a(args), plane(lds), q(q0)
    {
        if (!LDS) e = a.env0 + q % a.n;
        load();
    }
    __device__ __forceinline__ void load()
    {
        const int64_t qc = q < a.n_steps ? q : a.n_steps - 1;
        p = a.src[qc * a.src_stride];
        p = p < 0 ? 0 : p >= a.S ? a.S - 1 : p;  // (rows are the engine's own: in range; a guard for the index, not a rule)
        if (GRID && LDS) return;
        if (!GRID) {
            y = (int32_t)((uint32_t)p / (uint32_t)a.W);
            x = p - y * a.W;
            base = p + y * 2 * R;  // LDS: y * (W + 2R) + x, the top-left cell of the view in the padded plane
        }
        if (!LDS) {
            int64_t g = a.n_grids > 1 ? e / a.group : 0;
            g = g < a.n_grids ? g : a.n_grids - 1;
            flags = a.cell + g * a.grid_stride;
            kind = a.kind ? a.kind + g * a.kind_stride : nullptr;
        }
    }
    __device__ __forceinline__ void next()
    {
        ++q;
        if (!LDS) e = e + 1 == a.env0 + a.n ? a.env0 : e + 1;
        load();
    }
    // EGO: the cell dy, dx of the view
    __device__ __forceinline__ uint32_t ego(int32_t dy, int32_t dx) const
    {
        if (LDS) return plane[base + dy * (a.W + 2 * R) + dx];
        const int32_t yy = y + dy - R, xx = x + dx - R;
        if ((uint32_t)yy >= (uint32_t)a.H || (uint32_t)xx >= (uint32_t)a.W) return 4u;
        const int32_t s = yy * a.W + xx;
        return gu_tile_kind(kind, flags[s], s);
    }
    // GRID: cell s of the grid
    __device__ __forceinline__ uint32_t whole(int32_t s) const
    {
        const uint32_t c = LDS ? plane[s] : gu_tile_kind(kind, flags[s], s);
        return c + (s == p ? 8u : 0u);
    }
};

template <int R, bool GRID, bool LDS>
__device__ __forceinline__ void gu_sense_pieces(const SenseArgs &a, const uint8_t *plane)
{
    constexpr uint32_t K = 2 * R + 1, V2 = K * K;
    const uint32_t V = GRID ? (uint32_t)a.S : V2;
#pragma unroll 1
    for (int i = 0; i < GU_SENSE_PIECES; ++i) {
        const int64_t piece = ((int64_t)blockIdx.x * GU_SENSE_PIECES + i) * GU_SENSE_BLOCK + threadIdx.x;
        if (piece >= a.n_pieces) return;
        const uint32_t f0 = (uint32_t)(piece * 16);  // a call writes at most 2^32 bytes: the last piece begins below that
        const uint32_t q0 = GRID ? f0 / V : f0 / V2;
        uint32_t v = f0 - q0 * V;      // GRID: the cell; EGO: dy * K + dx
        int32_t dy = (int32_t)(v / K), dx = (int32_t)(v - (uint32_t)dy * K);
        SenseCursor<R, GRID, LDS> c(a, plane, (int64_t)q0);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t b = GRID ? c.whole((int32_t)v) : c.ego(dy, dx);
            w[j >> 2] |= b << (8 * (j & 3));
            if (GRID) {
                if (++v == V) {
                    v = 0;
                    c.next();
                }
            } else if (++dx == (int32_t)K) {
                dx = 0;
                if (++dy == (int32_t)K) {
                    dy = 0;
                    c.next();
                }
            }
        }
        *reinterpret_cast<uint4 *>(a.out + piece * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

template <int R, bool GRID>
__global__ void __launch_bounds__(GU_SENSE_BLOCK) gu_sense_kernel(const SenseArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t plane[GU_SENSE_LDS_BYTES];
    constexpr int64_t K = 2 * R + 1;
    const int64_t V = GRID ? (int64_t)a.S : K * K;
    // does one grid serve every env-step of this workgroup's chunk?  (the same answer in every lane)
    bool lds = (int64_t)(a.W + 2 * R) * (a.H + 2 * R) <= GU_SENSE_LDS_BYTES;
    int64_t g = 0;
    if (lds && a.n_grids > 1) {
        const int64_t f_lo = (int64_t)blockIdx.x * GU_SENSE_CHUNK, f_end = a.n_steps * V;
        const int64_t f_hi = f_lo + GU_SENSE_CHUNK < f_end ? f_lo + GU_SENSE_CHUNK : f_end;  // (bytes past the end repeat the last env-step)
        const int64_t q_lo = f_lo / V, q_hi = (f_hi - 1) / V;
        const int64_t t_lo = q_lo / a.n, t_hi = q_hi / a.n;
        g = (a.env0 + q_lo - t_lo * a.n) / a.group;
        lds = t_lo == t_hi && g == (a.env0 + q_hi - t_hi * a.n) / a.group && g < a.n_grids;
    }
    if (lds) {
        gu_sense_stage<R>(a, g, plane);
        gu_sense_pieces<R, GRID, true>(a, plane);
    } else {
        gu_sense_pieces<R, GRID, false>(a, plane);
    }
}

typedef void (*gu_sense_fn)(const SenseArgs);
static gu_sense_fn gu_sense_pick(int32_t mode, int32_t radius)
{
    if (mode == GU_SENSE_GRID) return gu_sense_kernel<0, true>;
    switch (radius) {
    case 0: return gu_sense_kernel<0, false>;
    case 1: return gu_sense_kernel<1, false>;
    case 2: return gu_sense_kernel<2, false>;
    case 3: return gu_sense_kernel<3, false>;
    case 4: return gu_sense_kernel<4, false>;
    case 5: return gu_sense_kernel<5, false>;
    case 6: return gu_sense_kernel<6, false>;
    default: return gu_sense_kernel<7, false>;
    }
}

// n_rows rows of n envs from env0 on, positions src[q * stride]; the views land in the engine's scratch and, when `view` is given,
// on the host.
static int gu_sense_launch(gu_engine *h, const int32_t *src, int32_t stride, int64_t n_rows, int64_t env0, int64_t n, int32_t mode,
                           int32_t radius, uint8_t *view)
{
    GU_REQUIRE(mode == GU_SENSE_EGO || mode == GU_SENSE_GRID, GU_ERR_INVALID, "unknown sensor mode %d", (int)mode);
    GU_REQUIRE(mode == GU_SENSE_GRID || (radius >= 0 && radius <= GU_SENSE_MAX_R), GU_ERR_INVALID, "radius %d outside 0..%d", (int)radius,
               GU_SENSE_MAX_R);
    const int64_t K = 2 * (int64_t)radius + 1, V = mode == GU_SENSE_GRID ? (int64_t)h->S : K * K;
    GU_REQUIRE(n_rows * n <= (1ll << 32) / V, GU_ERR_INVALID, "%lld views of %lld bytes are too many for one call", (long long)(n_rows * n),
               (long long)V);
    const int64_t bytes = n_rows * n * V, n_pieces = (bytes + 15) / 16;
    int rc = gu_ensure_scratch(h, (size_t)n_pieces * 16);
    if (rc != GU_OK) return rc;
    SenseArgs a{h->d_cell, h->d_kind, src, (uint8_t *)h->d_scratch, n_rows * n, n_pieces, env0, n, h->group > 0 ? h->group : h->N,
                2 * (int64_t)h->cell_bytes, (int64_t)h->cell_bytes, stride, h->W, h->H, h->S, h->n_grids};
    const int64_t blocks = (n_pieces + GU_SENSE_BLOCK * GU_SENSE_PIECES - 1) / (GU_SENSE_BLOCK * GU_SENSE_PIECES);
    hipLaunchKernelGGL(gu_sense_pick(mode, radius), dim3((unsigned)blocks), dim3(GU_SENSE_BLOCK), 0, h->stream, a);
    GU_HIP(hipGetLastError());
    if (view) {
        GU_HIP(hipMemcpyAsync(view, h->d_scratch, (size_t)bytes, hipMemcpyDeviceToHost, h->stream));
        GU_HIP(hipStreamSynchronize(h->stream));
    }
    return GU_OK;
}

extern "C" int gu_sense(gu_handle h, int64_t env0, int64_t n, int32_t mode, int32_t radius, uint8_t *view)
{
    int rc = gu_use_device(h);
    if (rc != GU_OK) return rc;
    GU_REQUIRE(h->has_grid, GU_ERR_STATE, "no grid set");
    GU_REQUIRE(env0 >= 0 && n > 0 && env0 + n <= h->N, GU_ERR_INVALID, "env range [%lld,%lld) outside the batch", (long long)env0,
               (long long)(env0 + n));
    return gu_sense_launch(h, h->pos() + env0, 1, 1, env0, n, mode, radius, view);
}

extern "C" int gu_sense_trajectory(gu_handle h, int64_t t0, int64_t T, int32_t mode, int32_t radius, uint8_t *view)
{
    int rc = gu_use_device(h);
    if (rc != GU_OK) return rc;
    GU_REQUIRE(h->has_grid, GU_ERR_STATE, "no grid set");
    GU_REQUIRE(h->d_traj && h->traj_kind != 0 && t0 >= 0 && T > 0 && t0 + T <= h->traj_T, GU_ERR_STATE,
               "rows [%lld,%lld) not in the trajectory buffer, or nothing written there yet", (long long)t0, (long long)(t0 + T));
    GU_REQUIRE(h->traj_kind != 2, GU_ERR_STATE, "the buffer holds a PACKED trajectory: the sensor reads int32 rows");
    const bool triples = h->traj_kind == 3;  // [T][N][3]: the obs word leads each triple; else the obs plane [T][N] comes first
    const int32_t *src = h->d_traj + (size_t)t0 * (size_t)h->N * (triples ? 3 : 1);
    return gu_sense_launch(h, src, triples ? 3 : 1, T, 0, h->N, mode, radius, view);
}
