// gu_rollout_greedy.hip -- instantiates the fused rollout kernel (gu_rollout.hpp) for GU_POLICY_GREEDY.
#include "gu_rollout.hpp"

bool gu_rollout_greedy(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &a) { return gu_rollout_general<GU_POLICY_GREEDY>(h, p, a); }
