// kernels_boundary.hip -- the signed Euclidean distance map of a label plane, exact, in two launches (boundary.h).
//
// G = { y > 0.5 } of one image.  For a pixel q of the plane, d2(q) is the smallest squared distance to a pixel of G (q outside G) or
// to a pixel of the plane outside G (q inside); phi(q) = sqrt(d2) outside, 1 - sqrt(d2) inside, 0 where the other set is empty.
//   boundary_cols   per pixel the rows to the nearest pixel of G in its column and to the nearest pixel outside G: two uint16 in one
//                   word (G low, the complement high), kSurfaceFar where the column has none.  k_surface_cols' scheme: a column's
//                   labels bit-packed into 32-row words in LDS, the nearest set bit by clz / ffs -- here of the word and of its
//                   complement, so one pass serves both sides
//   boundary_rows   d2(x, y) = min over x' of (x - x')^2 + g(x', y)^2, g the column distance to the OTHER set: the lower envelope of
//                   the row's parabolas, evaluated at every pixel.  The row's words go to LDS (rows above kBdRowsLds pixels are read
//                   from global memory); a pixel walks outward from x, one side after the other, and stops where (x - x')^2 alone
//                   reaches the best so far (k_surface_sample's walk), passing over every 32-pixel segment whose smallest
//                   column distance shows that it cannot win.  A row whose words all hold the sentinel for a side belongs to
//                   an image without that side (its columns are the plane's): no walk, d2 = 0, phi = 0
// Every value is an integer function of the labels (sqrt in double, rounded once to float): bit-identical from run to run.
#include <cstdint>

#include "boundary.h"
#include "kernels.h"
#include "region.h"

namespace dnnca {

namespace {

constexpr int kBdBlock = 256;
constexpr int kBdColsX = 16, kBdColsL = kBdBlock / kBdColsX;      // columns of a block, threads per column
constexpr int kBdRowsLds = 8192;                                  // a row of up to this many pixels is staged in LDS (32 KiB)
constexpr int kBdSeg = 32;                                        // pixels of a row segment: its smallest column distance prunes the walk
constexpr int kBdChunk = 8;                                       // pixels of a segment looked at between two exit tests
constexpr int kBdFar2 = (int)(kSurfaceFar * kSurfaceFar);

// the 32-row word `cc` of column `col`: the labels' bits, or (BG) those of the complement inside the plane
template <bool BG>
DEVINL uint32_t bd_word(const uint32_t* words, int cc, int col, int pieces, int H) {
    uint32_t o = words[cc * kBdColsX + col];
    if (BG) {
        o = ~o;
        if (cc == pieces - 1) o &= 0xffffffffu >> (pieces * 32 - H);
    }
    return o;
}

// rows from row c * 32 + j to the nearest set bit of the column's words of one side
template <bool BG>
DEVINL void bd_piece(const uint32_t* words, int c, int col, int pieces, int H, unsigned (&dist)[32]) {
    const uint32_t m = bd_word<BG>(words, c, col, pieces, H);
    int above = -1, below = -1;          // the nearest set row before and behind the piece
    for (int cc = c - 1; cc >= 0; --cc) {
        const uint32_t o = bd_word<BG>(words, cc, col, pieces, H);
        if (o) { above = cc * 32 + 31 - __clz((int)o); break; }
    }
    for (int cc = c + 1; cc < pieces; ++cc) {
        const uint32_t o = bd_word<BG>(words, cc, col, pieces, H);
        if (o) { below = cc * 32 + __ffs((int)o) - 1; break; }
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int y = c * 32 + j;
        const uint32_t upto = m & (0xffffffffu >> (31 - j)), from = m >> j;
        const int yu = upto ? c * 32 + 31 - __clz((int)upto) : above;
        const int yd = from ? y + __ffs((int)from) - 1 : below;
        const unsigned du = yu >= 0 ? (unsigned)(y - yu) : kSurfaceFar, dd = yd >= 0 ? (unsigned)(yd - y) : kSurfaceFar;
        dist[j] = min(du, dd);
    }
}

// a block takes kBdColsX columns of one image; thread (column, lane) takes the 32-row pieces lane, lane + kBdColsL, ... of its column
__global__ __launch_bounds__(kBdBlock) void k_boundary_cols(const float* __restrict__ Y, int H, int W, uint32_t* __restrict__ V) {
    extern __shared__ uint32_t words[];  // [pieces][kBdColsX]
    const int col = threadIdx.x & (kBdColsX - 1), lane = threadIdx.x / kBdColsX;
    const int x = (int)blockIdx.x * kBdColsX + col;
    const int pieces = (H + 31) / 32;
    const size_t at = (size_t)blockIdx.y * H * W + x;
    const float* yy = Y + at;
    uint32_t* v = V + at;
    for (int c = lane; c < pieces; c += kBdColsL) {
        uint32_t m = 0;
        if (x < W) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int y = c * 32 + j;
                if (y < H) m |= (uint32_t)(yy[(size_t)y * W] > 0.5f) << j;
            }
        }
        words[c * kBdColsX + col] = m;
    }
    __syncthreads();
    if (x >= W) return;
    for (int c = lane; c < pieces; c += kBdColsL) {
        unsigned df[32], db[32];
        bd_piece<false>(words, c, col, pieces, H, df);
        bd_piece<true>(words, c, col, pieces, H, db);
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int y = c * 32 + j;
            if (y < H) v[(size_t)y * W] = df[j] | (db[j] << 16);
        }
    }
}

// one side of a pixel's walk (DIR -1: towards x' = 0, +1: towards W - 1), segment by segment.  A side ends where (x - x')^2 alone
// reaches the best so far; a segment whose nearest pixel and smallest column distance together cannot beat it is passed over
template <int DIR>
DEVINL int bd_walk(const uint32_t* g, const uint32_t* segm, int x, int W, int sh, int best) {
    for (int xe = x + DIR; DIR < 0 ? xe >= 0 : xe < W;) {          // xe: the nearest pixel of this side not yet looked at
        const int dx0 = DIR < 0 ? x - xe : xe - x;
        if (dx0 * dx0 >= best) break;
        const int s = xe / kBdSeg;
        const int end = DIR < 0 ? s * kBdSeg : min(s * kBdSeg + kBdSeg - 1, W - 1);      // the segment's far pixel
        const int m = (int)((segm[s] >> sh) & 0xffffu);
        if (dx0 * dx0 + m * m < best) {
            // kBdChunk pixels at a time: independent loads, one exit test per chunk (a pixel too far to win only costs its look)
            for (int xx = xe; DIR < 0 ? xx >= end : xx <= end; xx += kBdChunk * DIR) {
                const int dxc = DIR < 0 ? x - xx : xx - x;
                if (dxc * dxc >= best) break;
#pragma unroll
                for (int u = 0; u < kBdChunk; ++u) {
                    const int xi = xx + u * DIR, dx = dxc + u;
                    if (DIR < 0 ? xi >= end : xi <= end) {
                        const int o = (int)((g[xi] >> sh) & 0xffffu);
                        best = min(best, dx * dx + o * o);
                    }
                }
            }
        }
        xe = end + DIR;
    }
    return best;
}

// a block takes one row of one image.  LDS: the row's words are staged behind the segment minima; else they are read where
// boundary_cols left them.  segm[s]: the smallest column distance of the row's pixels s * kBdSeg .. (both sides, packed as the words)
template <bool LDS>
__global__ __launch_bounds__(kBdBlock) void k_boundary_rows(const uint32_t* __restrict__ V, int H, int W, float* __restrict__ phi,
                                                            int* __restrict__ d2) {
    extern __shared__ uint32_t lds[];
    uint32_t* segm = lds;
    uint32_t* staged = lds + (W + kBdSeg - 1) / kBdSeg;
    const size_t at = ((size_t)blockIdx.y * H + blockIdx.x) * W;
    const uint32_t* row = V + at;
    int some_f = 0, some_b = 0;
    for (int x0 = 0; x0 < W; x0 += kBdBlock) {           // every thread makes every trip: the shuffles need whole lane groups
        const int x = x0 + (int)threadIdx.x;
        uint32_t v = kSurfaceFar | (kSurfaceFar << 16);
        if (x < W) {
            v = row[x];
            if (LDS) staged[x] = v;
        }
        unsigned lo = v & 0xffffu, hi = v >> 16;
#pragma unroll
        for (int o = kBdSeg / 2; o > 0; o >>= 1) {
            lo = min(lo, (unsigned)__shfl_xor((int)lo, o, 64));
            hi = min(hi, (unsigned)__shfl_xor((int)hi, o, 64));
        }
        if ((threadIdx.x & (kBdSeg - 1)) == 0 && x < W) segm[x / kBdSeg] = lo | (hi << 16);
        some_f |= lo != kSurfaceFar;
        some_b |= hi != kSurfaceFar;
    }
    some_f = __syncthreads_or(some_f);
    some_b = __syncthreads_or(some_b);
    const uint32_t* g = LDS ? staged : row;
    for (int x = threadIdx.x; x < W; x += kBdBlock) {
        const uint32_t v = g[x];
        const bool inside = (v & 0xffffu) == 0u;
        const int sh = inside ? 16 : 0;                 // a pixel of G looks for the complement, any other pixel for G
        const int g0 = (int)((v >> sh) & 0xffffu);
        int best = g0 * g0;
        if (inside ? some_b : some_f) {
            best = bd_walk<-1>(g, segm, x, W, sh, best);
            best = bd_walk<1>(g, segm, x, W, sh, best);
        }
        float f = 0.f;
        if (best >= kBdFar2) {
            best = 0;                                   // the other set is empty
        } else {
            const float d = (float)sqrt((double)best);
            f = inside ? 1.0f - d : d;
        }
        phi[at + x] = f;
        if (d2) d2[at + x] = best;
    }
}

}  // namespace

void boundary_transform(Model* m, const float* y, int B, int H, int W, uint32_t* cols, float* phi, int32_t* d2) {
    const double n = (double)B * H * W;
    LAUNCH(m, "boundary_cols", 8.0 * n, 0,
           hipLaunchKernelGGL(k_boundary_cols, dim3((W + kBdColsX - 1) / kBdColsX, B), dim3(kBdBlock),
                              (size_t)((H + 31) / 32) * kBdColsX * 4, m->stream, y, H, W, cols));
    const size_t segs = (size_t)(W + kBdSeg - 1) / kBdSeg;
    if (W <= kBdRowsLds)
        LAUNCH(m, "boundary_rows", (d2 ? 12.0 : 8.0) * n, 0,
               hipLaunchKernelGGL(k_boundary_rows<true>, dim3(H, B), dim3(kBdBlock), (segs + W) * 4, m->stream, cols, H, W, phi, d2));
    else
        LAUNCH(m, "boundary_rows", (d2 ? 12.0 : 8.0) * n, 0,
               hipLaunchKernelGGL(k_boundary_rows<false>, dim3(H, B), dim3(kBdBlock), segs * 4, m->stream, cols, H, W, phi, d2));
}

}  // namespace dnnca
