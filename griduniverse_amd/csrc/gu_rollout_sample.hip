// gu_rollout_sample.hip -- instantiates the fused rollout kernel (gu_rollout.hpp) for GU_POLICY_SAMPLE.
#include "gu_rollout.hpp"

bool gu_rollout_sample(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &a) { return gu_rollout_general<GU_POLICY_SAMPLE>(h, p, a); }
