// TEST INFRASTRUCTURE ONLY: the HOST form of the FM discriminator of m17hip_upload_iq — m17cxx/detail/core.h (fm_cross, fm_phase, fm_discriminate) compiled
// by the host compiler, the same text the kernel compiles.  One row of either IQ format with a gain and a carry in / out, and the two pieces on arrays
// for the tests of the arithmetic itself.  Built and loaded by tests/iq_lib.py (g++ -O2 -ffp-contract=off).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>

namespace core = mobilinkd::core;

extern "C" {

// iq: n interleaved I,Q samples (format 1: int16, 2: float32, as M17HIP_IQ_*); carry[2]: the sample in front of the row as floats, on return the row's last one
void iqo_discriminate(const void* iq, int format, size_t n, float gain, float* carry, float* out)
{
    float pi = carry[0], pq = carry[1];
    for (size_t k = 0; k < n; ++k) {
        float i, q;
        if (format == 1) { i = (float)((const int16_t*)iq)[2 * k]; q = (float)((const int16_t*)iq)[2 * k + 1]; }
        else { i = ((const float*)iq)[2 * k]; q = ((const float*)iq)[2 * k + 1]; }
        out[k] = core::fm_discriminate(i, q, pi, pq, gain);
        pi = i; pq = q;
    }
    carry[0] = pi; carry[1] = pq;
}
void iqo_cross(const float* i, const float* q, const float* pi, const float* pq, size_t n, float* re, float* im)
{
    for (size_t k = 0; k < n; ++k) core::fm_cross(i[k], q[k], pi[k], pq[k], re[k], im[k]);
}
void iqo_phase(const float* re, const float* im, size_t n, float* out)
{
    for (size_t k = 0; k < n; ++k) out[k] = core::fm_phase(re[k], im[k]);
}

}
