// The tile rule of resample_kernel as the library itself computes it (csrc/m17_resample_kernels.hpp: resample_groups, resample_q, resample_lds_bytes), for
// tests/test_resample_input.py to hold against resample_lib.tile, its restatement.  Host code only: no HIP call is made, it runs without a GPU.
//   resample_tile DECIM1 UP DOWN NTAPS1 NTAPS2 [DECIM1 UP DOWN NTAPS1 NTAPS2 ...]   ->   one line "G Q BYTES" per shape
#include <cstdio>
#include <cstdlib>

#include "m17_resample_kernels.hpp"

int main(int argc, char** argv)
{
    if (argc < 6 || (argc - 1) % 5) return 2;
    for (int i = 1; i < argc; i += 5) {
        const uint32_t R1 = (uint32_t)std::atoi(argv[i]), U = (uint32_t)std::atoi(argv[i + 1]), D = (uint32_t)std::atoi(argv[i + 2]);
        const uint32_t L1 = (uint32_t)std::atoi(argv[i + 3]), L2 = (uint32_t)std::atoi(argv[i + 4]);
        const uint32_t G = m17::resample_groups(L1, R1, L2, U, D), Q = m17::resample_q(L1, R1, L2, U, D, G);
        std::printf("%u %u %zu\n", G, Q, m17::resample_lds_bytes(L1, R1, L2, U, D, G, Q));
    }
    return 0;
}
