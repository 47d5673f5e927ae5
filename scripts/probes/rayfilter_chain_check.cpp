// rayfilter_chain_check.cpp -- the HOST build of the ray-filter chain (ohm_amd/csrc/ray_filter_chain.h) as a program of
// its own, for sanitizer runs without a GPU and without Python in the process:
//
//   g++ -std=c++14 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -static-libasan -static-libubsan -o rayfilter_chain_check scripts/probes/rayfilter_chain_check.cpp
//   ./rayfilter_chain_check cases.bin > results.txt
//
// cases.bin: any number of blocks { uint32 stage count; that many ohmhip_ray_filter_stage records; uint64 ray count;
// 6 doubles per ray }.  Output: a line "chain <index> <rays>" per block, then per ray "<keep> <flags>" and the six
// coordinates as the chain leaves them, as 16 hex digits of their bit patterns.  tests/test_rayfilter_chain_host.py
// writes the case list, runs this and compares with the model.
#include "../../ohm_amd/csrc/ray_filter_chain.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv)
{
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
    return 2;
  }
  std::FILE *in = std::fopen(argv[1], "rb");
  if (!in)
  {
    std::perror(argv[1]);
    return 2;
  }
  int status = 0;
  for (unsigned block = 0;; ++block)
  {
    uint32_t n_stages = 0;
    if (std::fread(&n_stages, sizeof(n_stages), 1, in) != 1)
    {
      break;  // end of the list
    }
    if (n_stages > OHMHIP_MAX_RAY_FILTER_STAGES)
    {
      status = 3;
      break;
    }
    std::vector<ohmhip_ray_filter_stage> stages(n_stages);
    uint64_t n_rays = 0;
    if ((n_stages && std::fread(stages.data(), sizeof(ohmhip_ray_filter_stage), n_stages, in) != n_stages) ||
        std::fread(&n_rays, sizeof(n_rays), 1, in) != 1)
    {
      status = 3;
      break;
    }
    std::vector<double> rays(size_t(n_rays) * 6);
    if (n_rays && std::fread(rays.data(), sizeof(double) * 6, size_t(n_rays), in) != size_t(n_rays))
    {
      status = 3;
      break;
    }
    std::printf("chain %u %" PRIu64 "\n", block, n_rays);
    for (size_t i = 0; i < size_t(n_rays); ++i)
    {
      double start[3] = { rays[6 * i], rays[6 * i + 1], rays[6 * i + 2] };
      double end[3] = { rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5] };
      unsigned flags = 0;
      const bool keep = ohmhip::rayFilterChain(stages.data(), n_stages, start, end, &flags);
      uint64_t bits[6];
      std::memcpy(bits, start, sizeof(start));
      std::memcpy(bits + 3, end, sizeof(end));
      std::printf("%d %u %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n",
                  keep ? 1 : 0, flags, bits[0], bits[1], bits[2], bits[3], bits[4], bits[5]);
    }
  }
  std::fclose(in);
  if (status)
  {
    std::fprintf(stderr, "%s: malformed block\n", argv[1]);
  }
  return status;
}
