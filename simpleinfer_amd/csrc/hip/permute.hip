// permute.hip -- the strided-gather copy of include/si_permute.h (Tensor.permute / reshape / view / torch.transpose / squeeze / unsqueeze) on
// fp32 and fp16 tensors.  Pure data movement: values travel as integer words, nothing here does arithmetic on a value.
//
// The host pads every nest to four loop dimensions (leading extents of 1) and hands the kernels 32-bit extents, input strides and output
// strides; it refuses nests whose element offsets or item counts do not fit 31 bits, so all index arithmetic is 32-bit and unsigned.
//
// permute_rows / permute_elem: a grid-stride loop over ITEMS of the output (si_grid_for: at most SI_PERMUTE_MAX_BLOCKS workgroups of 256
// lanes), an item being one 16-byte vector of a run (rows, V > 1) or one element.  Consecutive lanes take consecutive items of a run, then
// consecutive runs: a wave writes whole runs of the destination; it reads whole runs of the source when the innermost input stride is 1
// (rows) and a gather otherwise (elem).  An item's run index is split into the three outer loop indices by two 32-bit divisions.
//
// permute_tile: a grid-stride loop over TILES (at most SI_PERMUTE_TILE_MAX_BLOCKS workgroups of 256 lanes) of 64 x 64 elements of the two
// dimensions (j, last) -- j the loop dimension whose input stride is 1.  Four waves read 64 rows of the tile along j (one 256-byte / 128-byte
// line per wave-instruction), store them as rows of an LDS image, and after a barrier read the image by columns and write 64 rows along
// `last`.  A row of the image is 64 elements plus one 4-byte word: the column read of lane l then sits at word 65 l (fp32) / 33 l (fp16) plus
// a constant, 32 different banks in each 32-lane half (ds_read: bank = word % 32, conflicts count per half).  The row writes are consecutive
// words (fp32) / consecutive halves, two lanes per word (fp16).
//
// Register table per instantiation: DESIGN.md section 9k.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "si_hip_internal.h"
#include "si_permute.h"

namespace {

constexpr int PM_THREADS = 256;

// the integer word a <T, V> item travels as
template <typename T, int V> struct PmWord { typedef u32x4 type; };
template <> struct PmWord<float, 1> { typedef uint32_t type; };
template <> struct PmWord<_Float16, 1> { typedef uint16_t type; };

// ---- rows / elem --------------------------------------------------------------------------------------------------------------
struct ItemArgs {
    const void* in;
    void* out;
    unsigned d1, d2;            // extents of loop dimensions 1 and 2 of the padded nest (0 is what is left)
    unsigned s0, s1, s2, s3;    // input strides
    unsigned out_ld;
    unsigned per_run;           // items of one run: dims[3] / V
    unsigned total;             // items of the launch (< 2^31)
};

template <typename T, int V>
__device__ __forceinline__ void item_body(const ItemArgs& a) {
    typedef typename PmWord<T, V>::type W;
    const T* const in = static_cast<const T*>(a.in);
    T* const out = static_cast<T*>(a.out);
    const size_t stride = (size_t)gridDim.x * PM_THREADS;
    for (size_t it = (size_t)blockIdx.x * PM_THREADS + threadIdx.x; it < a.total; it += stride) {
        const unsigned i = (unsigned)it;
        const unsigned run = i / a.per_run, v = i - run * a.per_run;
        const unsigned q = run / a.d2, i2 = run - q * a.d2;
        const unsigned i0 = q / a.d1, i1 = q - i0 * a.d1;
        const unsigned src = i0 * a.s0 + i1 * a.s1 + i2 * a.s2 + v * V * a.s3;   // (V > 1 only with s3 == 1)
        *reinterpret_cast<W*>(out + run * a.out_ld + v * V) = *reinterpret_cast<const W*>(in + src);
    }
}

template <typename T, int V>
__global__ __launch_bounds__(PM_THREADS) void permute_rows(ItemArgs a) { item_body<T, V>(a); }

template <typename T>
__global__ __launch_bounds__(PM_THREADS) void permute_elem(ItemArgs a) { item_body<T, 1>(a); }

// ---- tile ---------------------------------------------------------------------------------------------------------------------
struct TileArgs {
    const void* in;
    void* out;
    unsigned R, C;              // extents of the input-contiguous dimension j and of the last (output-contiguous) dimension
    unsigned sC;                // input stride of the last dimension (dimension j's is 1)
    unsigned oR;                // output stride of dimension j (the last dimension's is 1)
    unsigned B1;                // extent of the inner batch dimension (the outer one is what is left)
    unsigned ib0, ib1, ob0, ob1;   // input / output strides of the two batch dimensions
    unsigned tR, tC;            // tiles along j and along last
    unsigned tiles;             // tiles of the launch
};

template <typename T>
__global__ __launch_bounds__(PM_THREADS) void permute_tile(TileArgs a) {
    typedef typename PmWord<T, 1>::type W;
    constexpr unsigned TS = SI_PERMUTE_TILE, PITCH = TS + 4 / sizeof(T);
    static_assert(TS == 64 && PM_THREADS == 256, "a wave is one tile row, four waves take four rows per step");
    __shared__ W image[TS * PITCH];
    const W* const in = static_cast<const W*>(a.in);
    W* const out = static_cast<W*>(a.out);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        unsigned q = t / a.tC;
        const unsigned c0 = (t - q * a.tC) * TS;
        const unsigned q2 = q / a.tR;
        const unsigned r0 = (q - q2 * a.tR) * TS;
        const unsigned b0 = q2 / a.B1, b1 = q2 - b0 * a.B1;
        const unsigned ibase = b0 * a.ib0 + b1 * a.ib1, obase = b0 * a.ob0 + b1 * a.ob1;
        {
            const unsigned r = r0 + lane;
#pragma unroll
            for (unsigned k = 0; k < TS; k += 4) {
                const unsigned c = c0 + k + wave;
                if (r < a.R && c < a.C) image[(k + wave) * PITCH + lane] = in[ibase + c * a.sC + r];
            }
        }
        __syncthreads();
        {
            const unsigned c = c0 + lane;
#pragma unroll
            for (unsigned k = 0; k < TS; k += 4) {
                const unsigned r = r0 + k + wave;
                if (r < a.R && c < a.C) out[obase + r * a.oR + c] = image[lane * PITCH + k + wave];
            }
        }
        __syncthreads();   // (the next pass overwrites the image)
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

// the nest padded to four dimensions: extents, input strides (0 where the extent is 1), output strides
struct Nest {
    unsigned d[4], s[4], o[4];
    int tile_j;   // the padded index of the loop dimension with input stride 1 and extent > 1 that is not the last one; -1: none
};

// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_permute(const SiPermuteDesc* d, Nest& n) {
    if (!d) return SI_E_BADARG;
    if (d->rank < 1 || d->rank > 4) return SI_E_BADARG;
    for (int k = 0; k < d->rank; ++k)
        if (d->dims[k] <= 0 || d->in_stride[k] <= 0) return SI_E_BADARG;
    if (d->out_ld < d->dims[d->rank - 1]) return SI_E_BADARG;
    if (d->form < SI_PERMUTE_FORM_AUTO || d->form > SI_PERMUTE_FORM_ELEM) return SI_E_BADARG;
    const int pad = 4 - d->rank;
    uint64_t max_in = 0, runs = 1;
    for (int k = 0; k < 4; ++k) {
        n.d[k] = k < pad ? 1u : (unsigned)d->dims[k - pad];
        n.s[k] = 0;
        if (n.d[k] > 1) {
            const uint64_t st = (uint64_t)d->in_stride[k - pad];
            if (st > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
            max_in += (uint64_t)(n.d[k] - 1) * st;   // < 2^62 per term, checked after every term
            if (max_in > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
            n.s[k] = (unsigned)st;
        }
        if (k < 3) {
            runs *= n.d[k];
            if (runs > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
        }
    }
    if (n.d[3] == 1) n.s[3] = 1;   // (a run of one element is contiguous whatever its stride says)
    if (runs * (uint64_t)d->out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;   // covers the item count: items <= runs * dims[rank-1]
    n.o[3] = 1;
    n.o[2] = (unsigned)d->out_ld;
    n.o[1] = n.o[2] * n.d[2];   // (<= runs * out_ld)
    n.o[0] = n.o[1] * n.d[1];
    n.tile_j = -1;
    for (int k = 2; k >= 0; --k)
        if (n.d[k] > 1 && n.s[k] == 1) n.tile_j = k;
    return 0;
}

enum Form { kRows = SI_PERMUTE_FORM_ROWS, kTile = SI_PERMUTE_FORM_TILE, kElem = SI_PERMUTE_FORM_ELEM };

// the form a checked nest takes; 0: the forced form is not eligible
int pick_form(const SiPermuteDesc* d, const Nest& n) {
    const bool rows_ok = n.s[3] == 1, tile_ok = !rows_ok && n.tile_j >= 0;
    switch (d->form) {
        case SI_PERMUTE_FORM_ROWS: return rows_ok ? kRows : 0;
        case SI_PERMUTE_FORM_TILE: return tile_ok ? kTile : 0;
        case SI_PERMUTE_FORM_ELEM: return kElem;
        default: break;
    }
    if (rows_ok) return kRows;
    if (tile_ok && n.d[n.tile_j] >= SI_PERMUTE_TILE_MIN && n.d[3] >= SI_PERMUTE_TILE_MIN) return kTile;
    return kElem;
}

// 16-byte vectors when the run length, the other strides, the output pitch and both pointers allow it
template <typename T>
bool rows_is_vec(const Nest& n, const void* src, const void* dst) {
    constexpr unsigned V = (unsigned)(16 / sizeof(T));
    return n.d[3] % V == 0 && n.s[0] % V == 0 && n.s[1] % V == 0 && n.s[2] % V == 0 && n.o[2] % V == 0 && si_aligned_to(src, 16) &&
           si_aligned_to(dst, 16);
}

template <typename T>
int run_permute(const SiPermuteDesc* d, const void* src, void* dst, si_stream_t stream) {
    Nest n;
    const int rc = check_permute(d, n);
    if (rc != 0) return rc;
    if (!src || !dst) return SI_E_BADARG;
    const int form = pick_form(d, n);
    if (form == 0) return SI_E_BADARG;
    constexpr int V = (int)(16 / sizeof(T));
    if (form == kTile) {
        const int j = n.tile_j;
        int b[2], nb = 0;
        for (int k = 0; k < 3; ++k)
            if (k != j) b[nb++] = k;
        TileArgs a;
        a.in = src; a.out = dst;
        a.R = n.d[j]; a.C = n.d[3];
        a.sC = n.s[3]; a.oR = n.o[j];
        a.B1 = n.d[b[1]];
        a.ib0 = n.s[b[0]]; a.ib1 = n.s[b[1]];
        a.ob0 = n.o[b[0]]; a.ob1 = n.o[b[1]];
        a.tR = (a.R + SI_PERMUTE_TILE - 1) / SI_PERMUTE_TILE;
        a.tC = (a.C + SI_PERMUTE_TILE - 1) / SI_PERMUTE_TILE;
        const uint64_t tiles = (uint64_t)n.d[b[0]] * n.d[b[1]] * a.tR * a.tC;   // <= the element count: fits 31 bits
        a.tiles = (unsigned)tiles;
        const unsigned grid = tiles < SI_PERMUTE_TILE_MAX_BLOCKS ? (unsigned)tiles : SI_PERMUTE_TILE_MAX_BLOCKS;
        hipLaunchKernelGGL((permute_tile<T>), dim3(grid), dim3(PM_THREADS), 0, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    }
    const bool vec = form == kRows && rows_is_vec<T>(n, src, dst);
    ItemArgs a;
    a.in = src; a.out = dst;
    a.d1 = n.d[1]; a.d2 = n.d[2];
    a.s0 = n.s[0]; a.s1 = n.s[1]; a.s2 = n.s[2]; a.s3 = n.s[3];
    a.out_ld = n.o[2];
    a.per_run = vec ? n.d[3] / V : n.d[3];
    const size_t total = (size_t)n.d[0] * n.d[1] * n.d[2] * a.per_run;
    a.total = (unsigned)total;
    static_assert(SI_PERMUTE_MAX_BLOCKS == 256 * 8, "si_grid_for's cap");
    const dim3 grid(si_grid_for(total, PM_THREADS));
    if (vec) hipLaunchKernelGGL((permute_rows<T, V>), grid, dim3(PM_THREADS), 0, (hipStream_t)stream, a);
    else if (form == kRows) hipLaunchKernelGGL((permute_rows<T, 1>), grid, dim3(PM_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((permute_elem<T>), grid, dim3(PM_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

template <typename T>
const char* name_of(const SiPermuteDesc* d, const void* src, const void* dst) {
    constexpr bool half = sizeof(T) == 2;
    Nest n;
    if (check_permute(d, n) != 0) return "none";
    switch (pick_form(d, n)) {
        case kRows:
            if (rows_is_vec<T>(n, src, dst)) return half ? "permute_rows<_Float16, 8>" : "permute_rows<float, 4>";
            return half ? "permute_rows<_Float16, 1>" : "permute_rows<float, 1>";
        case kTile: return half ? "permute_tile<_Float16>" : "permute_tile<float>";
        case kElem: return half ? "permute_elem<_Float16>" : "permute_elem<float>";
        default: return "none";
    }
}

}  // namespace

extern "C" {

int si_hip_permute_f32(const SiPermuteDesc* d, const void* src, void* dst, si_stream_t stream) { return run_permute<float>(d, src, dst, stream); }

int si_hip_permute_f16(const SiPermuteDesc* d, const void* src, void* dst, si_stream_t stream) { return run_permute<_Float16>(d, src, dst, stream); }

const char* si_hip_permute_kernel_name(const SiPermuteDesc* d, const void* src, const void* dst, int half) {
    return half ? name_of<_Float16>(d, src, dst) : name_of<float>(d, src, dst);
}

}  // extern "C"
