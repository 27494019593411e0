// mm_sample_tu.hip -- translation unit of the posterior path sampling (mm_kernel_sample.hip): the forward half of the item kernel,
// then the backward sampling walk.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_sample.hip"

namespace mm {

template <bool STAGE, int CW>
static int launch_sample_walk(int64_t B, int max_S1p, const RunParams &p, const SampleParams &sp, hipStream_t stream) {
    const size_t lds = STAGE ? size_t(2) * size_t(max_S1p) * sizeof(float) : 0;
    const unsigned groups = unsigned((sp.K + MM_SAMPLE_NW * CW - 1) / (MM_SAMPLE_NW * CW));
    if (groups > 65535u) return mm_fail(MM_ERR_UNSUPPORTED, "mm_samplepaths_f32: more than " + std::to_string(65535 * MM_SAMPLE_NW * CW) + " samples in one call");
    return mm_launch(mm_sample_kernel<STAGE, CW>, dim3(unsigned(B), groups), dim3(64 * (MM_SAMPLE_NW + 1)), lds, stream, p, sp);
}

// chains per wave: the fewest for which every workgroup of the call is resident at once (two workgroups per compute unit)
static int sample_cw(int64_t B, int K, int n_cus) {
    for (int cw = 1; cw < MM_SAMPLE_CW; cw *= 2)
        if (B * ((K + MM_SAMPLE_NW * cw - 1) / (MM_SAMPLE_NW * cw)) <= 2 * int64_t(n_cus)) return cw;
    return MM_SAMPLE_CW;
}

template <bool STAGE>
static int launch_sample_cw(int cw, int64_t B, int max_S1p, const RunParams &p, const SampleParams &sp, hipStream_t stream) {
    switch (cw) {
    case 1: return launch_sample_walk<STAGE, 1>(B, max_S1p, p, sp, stream);
    case 2: return launch_sample_walk<STAGE, 2>(B, max_S1p, p, sp, stream);
    case 4: return launch_sample_walk<STAGE, 4>(B, max_S1p, p, sp, stream);
    default: return launch_sample_walk<STAGE, 8>(B, max_S1p, p, sp, stream);
    }
}

int mm_launch_sample(int64_t B, int NW, int NI, bool bigv, size_t lds, bool stage, int max_S1p, int n_cus, const RunParams &p, const SampleParams &sp,
                     hipStream_t stream) {
    const int rc = item_instance("path sampling", NI, bigv, [&](auto I) {
        return mm_launch(mm_log_kernel<MODE_FB, decltype(I)::NI, 1, false, decltype(I)::BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p);
    });
    if (rc) return rc;
    const int cw = sample_cw(B, sp.K, n_cus);
    return stage ? launch_sample_cw<true>(cw, B, max_S1p, p, sp, stream) : launch_sample_cw<false>(cw, B, max_S1p, p, sp, stream);
}

}  // namespace mm
