// libpylda_hip.so - document kernels of the fused streaming families (qfuse, qfusek, qgroup): instantiations and launchers.
// (host side of the C ABI declared in include/pylda_hip.h; see host_internal.h for the map of the translation units)
#include "host_internal.h"
#include "estep_qfuse.h"
#include "estep_qfusek.h"
#include "estep_qgroup.h"

namespace pylda_host {

template <int NP, int RWL, int TWL>
static int launch_qfuse_np(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L)
{
    // (QfuseLds is 74,256 and 160,512 bytes, QfusekLds below at least 66,064: above 64 KiB, launch_kernel opts in on every launch)
    HIP_TRY(ctx, launch_kernel(estep_qfuse_kernel<NP, RWL, TWL>, dim3((unsigned)L.count), dim3(512), QfuseLds<NP, TWL>::total, st, p));
    return PYLDA_OK;
}

int launch_qfuse(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L)
{
#ifndef PYLDA_QF4_RWL
#define PYLDA_QF4_RWL 6
#endif
#ifndef PYLDA_QF4_TWL
#define PYLDA_QF4_TWL 2
#endif
    return ctx->ldk == 512 ? launch_qfuse_np<4, PYLDA_QF4_RWL, PYLDA_QF4_TWL>(ctx, st, p, L) : launch_qfuse_np<3, 8, 4>(ctx, st, p, L);
}

template <int NP>
static int launch_qfusek_np(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L)
{
    HIP_TRY(ctx, launch_kernel(estep_qfusek_kernel<NP>, dim3((unsigned)L.count), dim3(512), QfusekLds<NP>::total, st, p));
    return PYLDA_OK;
}

int launch_qfusek(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L)
{
    switch (ctx->ldk / 128) {
    case 5: return launch_qfusek_np<5>(ctx, st, p, L);
    case 6: return launch_qfusek_np<6>(ctx, st, p, L);
    case 7: return launch_qfusek_np<7>(ctx, st, p, L);
    case 8: return launch_qfusek_np<8>(ctx, st, p, L);
    }
    return fail(ctx, PYLDA_ERR_STATE, "no fused streaming kernel for table stride %d", ctx->ldk);
}

template <int TL>
static int launch_qgroup_tl(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L)
{
    HIP_TRY(ctx, launch_kernel(estep_qgroup_kernel<TL, 8>, dim3((unsigned)L.count), dim3(512), QgroupLds<TL>::total, st, p));      // (at most 64 KiB: QgroupLds)
    return PYLDA_OK;
}

int launch_qgroup(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L)
{
    if (ctx->ldk == 64) return launch_qgroup_tl<8>(ctx, st, p, L);
    if (ctx->ldk == 128) return launch_qgroup_tl<16>(ctx, st, p, L);
    if (ctx->ldk == 256) return launch_qgroup_tl<32>(ctx, st, p, L);
    return fail(ctx, PYLDA_ERR_STATE, "no group-fused streaming kernel for table stride %d", ctx->ldk);
}

}  // namespace pylda_host
