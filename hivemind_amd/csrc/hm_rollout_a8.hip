// hm_rollout_a8.hip — the single-launch search with the evaluator on native FP8 MFMA: the instantiations of k_rollout_a8
// (hm_rollout.hip: the search roles unchanged, serve_role_a8 around the serve form of narrow_position_a8) and their lookup.  Compiled
// once per search role (-DHM_ROLLOUT_MODE=0|1|2) like hm_rollout.hip, but in translation units of its own built like hm_net_a8.hip
// without packed fp32 VALU operations: the evaluator's scale-and-bias epilogues and quantisation steps are then the very instructions of
// rise_forward_a8, which the lockstep loop runs and whose priors the single launch must reproduce bit for bit.
#define HM_ROLLOUT_A8
#include "hm_rollout.hip"

#ifndef HM_ROLLOUT_MODE
#error "compile with -DHM_ROLLOUT_MODE=0|1|2"
#endif
namespace {
// -> the k_rollout_a8 instantiation for a trunk of `ctiles` * 32 channels (nullptr: none), by the rule of rollout_kernel(): only
// the 128-channel trunk without a 5x5 block leaves the 5x5 depthwise code out
template <int MODE>
const void* rollout_kernel_a8(int ctiles, int k5) {
    using namespace hms;
    if (ctiles == 4) return k5 ? reinterpret_cast<const void*>(k_rollout_a8<MODE, 4, true>) : reinterpret_cast<const void*>(k_rollout_a8<MODE, 4, false>);
    if (ctiles == 12) return reinterpret_cast<const void*>(k_rollout_a8<MODE, 12, true>);
    return nullptr;
}
}  // namespace
#define HM_ROLLOUT_A8_ENTRY_(m) hm_rollout_a8_kernel_mode##m
#define HM_ROLLOUT_A8_ENTRY(m) HM_ROLLOUT_A8_ENTRY_(m)
extern "C" const void* HM_ROLLOUT_A8_ENTRY(HM_ROLLOUT_MODE)(int ctiles, int k5) { return rollout_kernel_a8<HM_ROLLOUT_MODE>(ctiles, k5); }
