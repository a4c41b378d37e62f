// Host check of k_spmv_st_dma's staging map (macroc_amd/csrc/st_dma_map.h): the same functions the
// kernel calls, run over every tile of a few grids.  Stand-alone (no GPU, no library), so it can be
// built with -fsanitize=address,undefined (tests/test_st_dma_map_cpu.py does).
//   usage: st_dma_map_check nx ny nz [kc [pad_align]]
// (one rank's owned box; kc: planes per z-chunk, default nz; pad_align as the library's padded layout:
//  1 (default) = row pitch PX a multiple of 16 nodes and x 104 bytes into its 16-byte-aligned
//  allocation, so 8 mod 16 and the staged rows shifted by one double; 2 = the same pitch, x at the
//  allocation's start; 0 = PX = nx + 2, x at the start)
// Checks, for every 64 x 16 tile of the box:
//   1. every ring element a marched node's rows read is written by exactly one (wave, piece, lane),
//      from the padded-plane element the row means;
//   2. source addresses are 16-byte aligned and inside the plane's record, which itself stays inside
//      the vector's allocation (pad_off bytes ahead, 256 - pad_off behind), or exactly ST_DMA_OOB;
//   3. no pair straddles a staged row;
//   4. no piece leaves its slot;
//   5. under the kernel's schedule, a slot is never written while a plane still to be read sits in
//      it, and every plane a step reads is in the ring.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../macroc_amd/csrc/st_dma_map.h"

static int fails = 0;
#define CHECK(c, ...)                         \
  do {                                        \
    if (!(c)) {                               \
      if (fails++ < 20) {                     \
        std::fprintf(stderr, "FAIL %s: ", #c); \
        std::fprintf(stderr, __VA_ARGS__);    \
        std::fprintf(stderr, "\n");           \
      }                                       \
    }                                         \
  } while (0)

static void check_tile(int nx, int ny, int PX, int pad_off, int i0, int j0) {
  const int PY = ny + 2, sft = (pad_off / 8) & 1;
  const long rec = st_dma_rec_bytes((long)PX * PY, sft);  // bytes of a padded plane's buffer record
  // the record inside the allocation: the first plane's starts at pad_off - lead >= 0, the last plane's
  // ends at most 256 - pad_off bytes past the vector; and every record 16-byte aligned
  CHECK(pad_off - st_dma_rec_lead(sft) >= 0 && (pad_off - st_dma_rec_lead(sft)) % 16 == 0, "record lead %d", pad_off);
  CHECK(rec - st_dma_rec_lead(sft) - 24L * PX * PY <= 256 - pad_off, "record tail past the allocation");
  CHECK((24L * PX * PY) % 16 == 0, "planes keep the alignment");
  const int len = 3 * (ST_DMA_TX + 2 < nx + 2 - i0 ? ST_DMA_TX + 2 : nx + 2 - i0);
  const int rows = ST_DMA_TY + 2 < ny + 2 - j0 ? ST_DMA_TY + 2 : ny + 2 - j0;
  // the slot image: for every double of a slot, how often it is written and from which padded element
  std::vector<int> cnt(ST_DMA_SLOT, 0);
  std::vector<long> from(ST_DMA_SLOT, -1);
  for (int w = 0; w < ST_DMA_WAVES; w++)
    for (int m = 0; m < 2; m++) {
      const int pc = st_dma_piece(w, m);
      if (!st_dma_piece_ok(pc)) continue;
      const int d0 = st_dma_dst(pc);
      CHECK(d0 >= 0 && d0 + ST_DMA_PIECE <= ST_DMA_SLOT && d0 % 2 == 0, "piece %d leaves its slot", pc);  // 4.
      for (int l = 0; l < 64; l++) {
        const unsigned s = st_dma_src(pc, l, i0, j0, PX, len, rows, sft);
        const int e = d0 + 2 * l;  // the lane's two doubles within the slot
        CHECK(e + 1 < ST_DMA_SLOT, "lane %d of piece %d leaves its slot", l, pc);
        if (e + 1 >= ST_DMA_SLOT) continue;
        cnt[e]++, cnt[e + 1]++;
        if (s == ST_DMA_OOB) continue;
        CHECK(s % 16 == 0 && (long)s + 16 <= rec, "source %u of (%d, %d): record %ld", s, pc, l, rec);  // 2.
        CHECK(e / ST_DMA_RL == (e + 1) / ST_DMA_RL, "pair %d straddles a staged row", e);              // 3.
        from[e] = (long)s / 8 - sft, from[e + 1] = (long)s / 8 - sft + 1;  // doubles from the plane's start
      }
    }
  for (int e = 0; e < ST_DMA_SLOT; e++) CHECK(cnt[e] == 1, "slot double %d written %d times", e, cnt[e]);
  // 1. the reads of the marched nodes: lane (lx, ly) of the tile, rows dy = -1 .. 1, 9 doubles from 3 lx
  for (int ly = 0; ly < ST_DMA_TY && j0 + ly < ny; ly++)
    for (int lx = 0; lx < ST_DMA_TX && i0 + lx < nx; lx++)
      for (int dy = -1; dy <= 1; dy++)
        for (int q = 0; q < 9; q++) {
          const int e = st_dma_read0(lx, ly, sft) + (1 + dy) * ST_DMA_RL + q;
          // padded node (i0 + lx + q / 3, j0 + ly + 1 + dy), component q % 3
          const long want = 3L * ((i0 + lx + q / 3) + (long)(j0 + ly + 1 + dy) * PX) + q % 3;
          CHECK(e < ST_DMA_PLANE && cnt[e] == 1 && from[e] == want, "read %d of node (%d, %d): from %ld, want %ld", e,
                i0 + lx, j0 + ly, from[e], want);
        }
}

// 5. the ring under the kernel's schedule, planes k0-1 .. of one z-chunk [k0, k1)
static void check_schedule(int k0, int k1) {
  int held[ST_DMA_SLOTS];  // the plane a slot holds (INT_MIN-like: nothing)
  const int NONE = -1000000;
  for (int s = 0; s < ST_DMA_SLOTS; s++) held[s] = NONE;
  auto issue = [&](int p, int last_read_of_old) {
    const int s = st_dma_slot(p, k0);
    CHECK(s >= 0 && s < ST_DMA_SLOTS, "slot %d of plane %d", s, p);
    // the plane it replaces is read no more: every later read is of a plane > last_read_of_old
    CHECK(held[s] == NONE || held[s] <= last_read_of_old, "plane %d overwrites plane %d still to be read", p, held[s]);
    for (int t = 0; t < ST_DMA_SLOTS; t++) CHECK(t == s || held[t] != p, "plane %d twice in the ring", p);
    held[s] = p;
  };
  auto reads = [&](int p) { CHECK(held[st_dma_slot(p, k0)] == p, "plane %d not in its slot", p); };
  for (int s = 0; s < 4; s++) issue(k0 - 1 + s, NONE);  // prologue
  for (int k = k0; k < k1; k += 2) {
    const bool more = k + 2 < k1;
    if (more) issue(k + 3, k - 2);  // top of the step: planes < k-1 are dead
    reads(k - 1), reads(k);         // rows 0 .. 2
    if (more) issue(k + 4, k - 1);  // after the mid-step barrier: plane k-1 is dead
    reads(k), reads(k + 1), reads(k + 2);  // rows 3 .. 8 (the planes issued in this step are not read in it)
  }
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s nx ny nz [kc [pad_align]]\n", argv[0]);
    return 2;
  }
  const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), nz = std::atoi(argv[3]);
  const int kc = argc > 4 ? std::atoi(argv[4]) : nz, pad_align = argc > 5 ? std::atoi(argv[5]) : 1;
  if (nx < 1 || ny < 1 || nz < 1 || kc < 1 || pad_align < 0 || pad_align > 2) {
    std::fprintf(stderr, "nx, ny, nz, kc >= 1, pad_align 0 .. 2\n");
    return 2;
  }
  const int PX = pad_align ? (nx + 2 + 15) / 16 * 16 : nx + 2, pad_off = pad_align == 1 ? 104 : 0;
  if (PX % 2) {
    std::fprintf(stderr, "odd row pitch %d: not eligible\n", PX);
    return 2;
  }
  int tiles = 0;
  for (int j0 = 0; j0 < ny; j0 += ST_DMA_TY)
    for (int i0 = 0; i0 < nx; i0 += ST_DMA_TX) check_tile(nx, ny, PX, pad_off, i0, j0), tiles++;
  for (int k0 = 0; k0 < nz; k0 += kc) check_schedule(k0, k0 + kc < nz ? k0 + kc : nz);
  std::printf("%d x %d x %d, kc %d, pitch %d, shift %d: %d tiles, %d failures\n", nx, ny, nz, kc, PX, (pad_off / 8) & 1, tiles,
              fails);
  return fails ? 1 : 0;
}
