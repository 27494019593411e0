// mm_quad_tu.hip -- translation unit of the quad kernels (mm_kernel_quad.hip): their instances and launches.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_quad.hip"

namespace mm {

template <int KQ, int RPT, int PASS>
static int launch_quad_kq_rpt(const QuadLaunch *h, const RunParams &p, hipStream_t stream) {
    return mm_launch(mm_fbq_kernel<KQ, RPT, PASS>, dim3(unsigned(h->B)), dim3(64 * h->nw), h->lds, stream, p);
}

template <int KQ, int PASS>
static int launch_quad_kq(const QuadLaunch *h, const RunParams &p, hipStream_t stream) {
    // rows per thread = ceil(max S1 / threads): 2 register-carried rows when that is enough
    const int NT = 64 * h->nw, rows = (h->max_S1p + NT - 1) / NT;
    if (rows <= 2) return launch_quad_kq_rpt<KQ, 2, PASS>(h, p, stream);
    return launch_quad_kq_rpt<KQ, 3, PASS>(h, p, stream);
}

template <int PASS>
static int launch_quad_pass(const QuadLaunch *h, const RunParams &p, hipStream_t stream) {
    switch (h->kq) {
        // one instance per KQ of the lists in mm_pack.h (what quad_kq_has_instance() answers by)
#define MM_QUAD_CASE(k) \
    case k: return launch_quad_kq<k, PASS>(h, p, stream);
        MM_QUAD_KQ_16WAVES(MM_QUAD_CASE)
        MM_QUAD_KQ_8WAVES(MM_QUAD_CASE)
#undef MM_QUAD_CASE
        default: return MM_ERR_UNSUPPORTED;
    }
}

int mm_launch_quad_pass(int pass, const QuadLaunch &ql, const RunParams &p, hipStream_t stream) {
    return pass == 0 ? launch_quad_pass<0>(&ql, p, stream) : launch_quad_pass<1>(&ql, p, stream);
}

}  // namespace mm
