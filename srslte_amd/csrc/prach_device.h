// prach_device.h -- kernel parameter block and launchers of prach_kernels.hip (PRACH detection, preamble formats 0 .. 3)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace phyhip {
namespace prach {

constexpr int kNzc     = 839;  // N_zc of the long formats
constexpr int kFirst   = 1536; // N_ifft_prach = kFirst * D: the length of the pruned first stage
constexpr int kMaxOcc  = 8;
constexpr int kRecHead = 4; // words of a root's record in front of its windows: corr_ave, Re / Im of the cross sum, one spare

// A root's record: kRecHead words, then n_wins peak values (float) and n_wins peak offsets (uint32).
struct Params {
  const float2*  sig;       // [n_occ][N]: the first N_ifft_prach samples of every occasion
  double2*       streams;   // [n_occ][D][839]: what the first stage keeps of F_d, in the order of the wanted bins
  const double2* tw_first;  // e^{-j 2 pi i / 1536}
  const double2* tw_n;      // e^{-j 2 pi i / N}
  const float2*  tw_zc;     // e^{-j 2 pi i / 839}
  const float2*  root_spec; // [n_search][839]
  uint32_t*      rec;       // [n_occ][n_search][rec_words]
  float2*        bins_out;  // [n_occ][839] or nullptr
  float*         corr_out;  // [n_occ][n_search][839] or nullptr
  int            N, D, n_occ, n_search, n_wins, N_cs, rec_words;
  double         norm;        // 1 / sqrt(N)
  int            k0[kMaxOcc]; // transform bin of caller bin `begin`: (begin + N / 2) mod N (forward mirror plan, dft_kernels.hip post_index)
};

hipError_t launch(const Params& p, hipStream_t stream); // the two kernels of a detection, in stream order
// object creation: spec[r] = the forward 839-point DFT with norm of seq[r], r < n_roots
hipError_t launch_root_spectra(const float2* seq, float2* spec, int n_roots, hipStream_t stream);

} // namespace prach
} // namespace phyhip
