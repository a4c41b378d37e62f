// Staging map of k_spmv_st_dma (the default-stencil march with direct-to-LDS loads): which 16 bytes
// of a padded x plane every (wave, piece, lane) brings into the 5-slot x ring.  The kernel and the
// host check (tests/csrc/st_dma_map_check.cpp) call the same functions.
//
// A staged plane is PR = 18 rows of RL = 208 doubles (k_spmv_st's layout: 66 nodes of a 64-wide tile
// row and its two x neighbours, padded to 16 mod 32 doubles).  One direct-to-LDS buffer load of 16
// bytes per lane writes 64 x 16 = 1,024 contiguous bytes, a piece of 128 doubles: a plane is 30
// pieces (the last one partly past the plane's 3,744 doubles), a ring slot is those 30 KiB.  Wave w
// of the block's 16 issues pieces w and w + 16 (the latter while it is below 30).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ST_DMA_HD __host__ __device__
#else
#define ST_DMA_HD
#endif

constexpr int ST_DMA_TX = 64, ST_DMA_TY = 16;            // the tile
constexpr int ST_DMA_RL = 208, ST_DMA_PR = ST_DMA_TY + 2;  // staged row length (doubles), rows per plane
constexpr int ST_DMA_PLANE = ST_DMA_PR * ST_DMA_RL;      // 3,744 doubles
constexpr int ST_DMA_PIECE = 128;                        // doubles one wave instruction writes
constexpr int ST_DMA_NPIECE = (ST_DMA_PLANE + ST_DMA_PIECE - 1) / ST_DMA_PIECE;  // 30
constexpr int ST_DMA_SLOT = ST_DMA_NPIECE * ST_DMA_PIECE;  // ring slot stride: 3,840 doubles = 30,720 B
constexpr int ST_DMA_SLOTS = 5;                          // plane p of a block sits in slot (p - k0 + 1) mod 5
constexpr int ST_DMA_WAVES = 16;
constexpr unsigned ST_DMA_OOB = 0x80000000u;             // a buffer offset past every record: loads 0
static_assert(ST_DMA_RL % 2 == 0, "an element pair never straddles a staged row");
static_assert(3 * (ST_DMA_TX + 2) + 1 <= ST_DMA_RL, "a shifted row fits the staged row");
static_assert(ST_DMA_NPIECE <= 2 * ST_DMA_WAVES, "two pieces per wave cover a plane");

// the pieces of wave w: w and w + 16; the second exists while it lies inside the slot
ST_DMA_HD inline int st_dma_piece(int wave, int m) { return wave + ST_DMA_WAVES * m; }
ST_DMA_HD inline bool st_dma_piece_ok(int piece) { return piece < ST_DMA_NPIECE; }

// first double of a piece within its slot (wave-uniform; lane l writes doubles 2 l, 2 l + 1 of the piece)
ST_DMA_HD inline int st_dma_dst(int piece) { return ST_DMA_PIECE * piece; }

// A lane's 16 source bytes must be 16-byte aligned.  The padded vectors start pad_off bytes into a
// 16-byte-aligned allocation (104 by default: x is 8 mod 16), so the staged rows are shifted by
// sft = (address of x / 8) mod 2 doubles: column o of a staged row sits at row position o + sft, the
// plane's buffer record starts 8 sft bytes before the plane and is 16 sft bytes longer than it (the
// pair at a row's end then reads one double past the row: inside the allocation, never used).
//
// byte offset into that record of the pair (piece, lane): staged element e = 128 piece + 2 lane is row
// position q = o + sft of staged row rr.  (i0, j0): the tile's first node, PX: the padded row pitch in
// nodes (even), len = 3 min(66, nx + 2 - i0) doubles of a row and rows = min(18, ny + 2 - j0) rows
// exist in the padded box; everything else is ST_DMA_OOB (the load returns zeros)
ST_DMA_HD inline unsigned st_dma_src(int piece, int lane, int i0, int j0, int PX, int len, int rows, int sft) {
  const int e = ST_DMA_PIECE * piece + 2 * lane;
  const int rr = e / ST_DMA_RL, q = e - rr * ST_DMA_RL;
  return e >= ST_DMA_PLANE || q >= len + sft || rr >= rows ? ST_DMA_OOB : 8u * (unsigned)(3 * (i0 + (j0 + rr) * PX) + q);
}

// the record of a padded plane of PXY nodes: bytes ahead of the plane, and its size
ST_DMA_HD inline int st_dma_rec_lead(int sft) { return 8 * sft; }
ST_DMA_HD inline long long st_dma_rec_bytes(long long PXY, int sft) { return 24 * PXY + 16 * sft; }

// first double a lane reads in a slot: staged row ly + 1 + dy (dy = -1), node lx's three columns
ST_DMA_HD inline int st_dma_read0(int lx, int ly, int sft) { return ly * ST_DMA_RL + 3 * lx + sft; }

// ring slot of plane p (p = k0 - 1 ... ) of a block whose chunk starts at plane k0
ST_DMA_HD inline int st_dma_slot(int p, int k0) { return (p - k0 + 1) % ST_DMA_SLOTS; }
