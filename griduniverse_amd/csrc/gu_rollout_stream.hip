// gu_rollout_stream.hip -- instantiates the fused rollout kernel (gu_rollout.hpp) for GU_POLICY_STREAM.
#include "gu_rollout.hpp"

bool gu_rollout_stream(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &a) { return gu_rollout_general<GU_POLICY_STREAM>(h, p, a); }
