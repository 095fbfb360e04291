// gu_rollout_uniform.hip -- instantiates the fused rollout kernel (gu_rollout.hpp) for GU_POLICY_UNIFORM.
#include "gu_rollout.hpp"

bool gu_rollout_uniform(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &a) { return gu_rollout_general<GU_POLICY_UNIFORM>(h, p, a); }
