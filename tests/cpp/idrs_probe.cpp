// The generated shadow block of hifamd_idrs_batch (P == NULL) from the host twin of the probe generator
// (hifir_amd/csrc/import.hpp nsp_probe_value): entry (i, j), j < s, from counter 16 i + j + 1, the imaginary part of a complex
// entry from counter 16 (n + i) + j + 1.  Writes the n * s real parts, then (cplx != 0) the n * s imaginary parts, row by
// row as raw doubles, for tests/test_idrs_host.py to hold idrs_util.generated_P against.
// Build: g++ -std=c++17 -O1 -pthread -I hifir_amd/csrc tests/cpp/idrs_probe.cpp;  run: idrs_probe n s seed cplx out.bin
#include "import.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
  if (argc != 6) return 2;
  const int64_t n = std::atoll(argv[1]), s = std::atoll(argv[2]);
  const uint64_t seed = std::strtoull(argv[3], nullptr, 0);
  const int cplx = std::atoi(argv[4]);
  std::FILE *f = std::fopen(argv[5], "wb");
  if (!f) return 3;
  for (int part = 0; part <= (cplx ? 1 : 0); ++part)
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < s; ++j) {
        const double v = hifamd::nsp_probe_value(seed, (uint64_t)(16 * ((part ? n : 0) + i) + j) + 1);
        if (std::fwrite(&v, sizeof v, 1, f) != 1) return 4;
      }
  return std::fclose(f) == 0 ? 0 : 5;
}
