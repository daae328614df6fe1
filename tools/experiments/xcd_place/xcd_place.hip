// Where do the blocks of consecutive launches land?  The c2 step is six launches on one stream whose kernels map
// blockIdx & 7 to an eighth of the rows (xcd_remap.h), on the assumption that the class blockIdx & 7 sits on the same
// XCD in every launch.  This program launches a trivial kernel at the step's six grids, in the step's order, and lane 0
// of every block stores the XCD it runs on (HW_REG_XCC_ID) to ids[launch][blockIdx.x].  The host then answers, per
// sequence of grids:
//   rr     is xcc(b) == (xcc(0) + b) & 7 for every block of a launch?                (violating blocks)
//   fixed  launches whose xcc(0) equals the previous launch's xcc(0)
//   cont   launches whose xcc(0) equals (previous xcc(0) + previous grid) & 7: dealing goes on where the last grid stopped
//   other  neither
// Sequences: the step's grids as they are, the same rounded up to multiples of 8, and the step's grids with a second
// grid dimension (members = 3), and the first once more at the end.  Each is run with an empty kernel, with one that
// holds 40 KB of LDS and spins about 2 us, so that the grid is more than one resident round and blocks queue as the real
// kernels' do, and with the two alternating from launch to launch, as the step alternates its kernels.
//   hipcc -O3 --offload-arch=gfx950 xcd_place.hip -o xcd_place && ./xcd_place out.tsv
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

constexpr int kMaxGrid = 1568, kLaunches = 6;

template <bool BUSY>
__global__ __launch_bounds__(256) void k_where(int *ids, int spin) {
  __shared__ int pad[BUSY ? 10240 : 1];
  if (BUSY) {
    pad[threadIdx.x] = spin;
    for (int i = 0; i < spin; ++i) __builtin_amdgcn_s_sleep(8);
    __syncthreads();
  }
  if (threadIdx.x == 0 && blockIdx.y == 0) {
    int id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(id));
    ids[blockIdx.x] = id + (BUSY ? pad[0] - spin : 0);
  }
}

struct Seq { const char *name; int grid[kLaunches]; int members; };

int main(int argc, char **argv) {
  const int rounds = 300;
  const char *kname[] = {"empty", "busy", "mixed"};
  const Seq seqs[] = {
      {"step", {1251, 1563, 1563, 1563, 1563, 1251}, 1},
      {"step_rounded_to_8", {1256, 1568, 1568, 1568, 1568, 1256}, 1},
      {"step_members_3", {1251, 1563, 1563, 1563, 1563, 1251}, 3},
      {"rounded_members_3", {1256, 1568, 1568, 1568, 1568, 1256}, 3},
      {"step_again", {1251, 1563, 1563, 1563, 1563, 1251}, 1},
  };
  FILE *f = argc > 1 ? std::fopen(argv[1], "w") : stdout;
  if (!f) { std::perror("open"); return 1; }
  const size_t n = (size_t)rounds * kLaunches * kMaxGrid;
  int *d = nullptr;
  CHECK(hipMalloc(&d, n * sizeof(int)));
  std::vector<int> h(n);
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  std::fprintf(f, "sequence\tkernel\tlaunch\tgrid\tlaunches\trr_violating_blocks\tfixed\tcont\tother\txcc0_histogram\n");
  for (const Seq &s : seqs) {
    for (int busy = 0; busy < 3; ++busy) {              // 2: the two kernels alternate
      CHECK(hipMemsetAsync(d, 0xff, n * sizeof(int), st));
      for (int r = 0; r < rounds; ++r)
        for (int l = 0; l < kLaunches; ++l) {
          int *p = d + ((size_t)r * kLaunches + l) * kMaxGrid;
          dim3 g(s.grid[l], s.members);
          if (busy == 1 || (busy == 2 && l % 2 == 0)) k_where<true><<<g, 256, 0, st>>>(p, 10);
          else k_where<false><<<g, 256, 0, st>>>(p, 0);
        }
      CHECK(hipGetLastError());
      CHECK(hipStreamSynchronize(st));
      CHECK(hipMemcpy(h.data(), d, n * sizeof(int), hipMemcpyDeviceToHost));
      long tot_fixed = 0, tot_cont = 0, tot_other = 0, tot_viol = 0;
      for (int l = 0; l < kLaunches; ++l) {
        long viol = 0, fixed = 0, cont = 0, other = 0, hist[8] = {0};
        for (int r = 0; r < rounds; ++r) {
          const int *p = h.data() + ((size_t)r * kLaunches + l) * kMaxGrid;
          const int x0 = p[0];
          if (x0 < 0 || x0 > 7) { std::fprintf(stderr, "bad id %d\n", x0); return 1; }
          ++hist[x0];
          for (int b = 0; b < s.grid[l]; ++b) viol += p[b] != ((x0 + b) & 7);
          if (r == 0 && l == 0) continue;                    // no previous launch of this sequence
          const int pl = l == 0 ? kLaunches - 1 : l - 1, pr = l == 0 ? r - 1 : r;
          const int px0 = h[((size_t)pr * kLaunches + pl) * kMaxGrid];
          const int pgrid = s.grid[pl] * s.members;
          const bool is_fixed = x0 == px0, is_cont = x0 == ((px0 + pgrid) & 7);
          // a previous grid that is a multiple of 8 makes the two the same: counted as both
          fixed += is_fixed; cont += is_cont; other += !is_fixed && !is_cont;
        }
        std::fprintf(f, "%s\t%s\t%d\t%dx%d\t%d\t%ld\t%ld\t%ld\t%ld\t", s.name, kname[busy], l, s.grid[l],
                     s.members, rounds, viol, fixed, cont, other);
        for (int i = 0; i < 8; ++i) std::fprintf(f, "%ld%s", hist[i], i == 7 ? "\n" : ",");
        tot_fixed += fixed; tot_cont += cont; tot_other += other; tot_viol += viol;
      }
      std::printf("%-20s %-5s rr_violations %ld fixed %ld cont %ld other %ld\n", s.name, kname[busy], tot_viol,
                  tot_fixed, tot_cont, tot_other);
    }
  }
  if (f != stdout) std::fclose(f);
  CHECK(hipFree(d));
  return 0;
}
