// rollout_plan_host.cpp -- gu_rollout_plan (csrc/gu_rollout_plan.hpp) without a device: reads "n_cu lds_per_cu" and then one case per
// line (the input columns of tests/golden/rollout_plan.json) from standard input, prints the twelve form words of each plan.
// Built by tests/test_rollout_plan.py with `hipcc -x hip --cuda-host-only` together with csrc/gu_options.hip.
#include "../griduniverse_amd/csrc/gu_rollout_plan.hpp"

#include <cstdarg>
#include <cstdio>

int gu_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    return code;
}

int main()
{
    // the option columns, in the order of tools/rollout_plan_table.py: OPTS
    const int option[] = {GU_OPT_ROLLOUT_BLOCK, GU_OPT_ROLLOUT_ROWS, GU_OPT_ROWS_COPIES, GU_OPT_ROLLOUT_MULTI, GU_OPT_ROLLOUT_MULTI_K, GU_OPT_ROLLOUT_MULTI_COPIES,
                          GU_OPT_ROLLOUT_XCD, GU_OPT_TRAJ_LAYOUT, GU_OPT_ROLLOUT_HALF_WAVES, GU_OPT_ROLLOUT_PACE, GU_OPT_ROLLOUT_ENTRY, GU_OPT_PACE_RECORD};
    enum { N, W, H, GRIDS, MULTI_START, POLICY, FLAGS, T, WIND, GUST, TRAIL, STRADDLE, ENTRY, OPT0, COLUMNS = OPT0 + sizeof option / sizeof option[0] };
    long long n_cu = 0, lds_per_cu = 0, v[COLUMNS];
    if (scanf("%lld %lld", &n_cu, &lds_per_cu) != 2) return 2;
    for (;;) {
        for (int i = 0; i < COLUMNS; ++i)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 2;
        gu_engine h;
        for (int64_t &o : h.opt) o = GU_OPT_UNSET;
        h.n_cu = (int)n_cu;
        h.lds_per_cu = lds_per_cu;
        h.N = v[N];
        h.has_grid = true;
        h.W = (int32_t)v[W], h.H = (int32_t)v[H], h.S = h.W * h.H;
        h.cell_bytes = (h.S + 15) & ~15;
        h.n_grids = (int32_t)v[GRIDS];
        h.group = h.N / h.n_grids;
        h.all_single_start = v[MULTI_START] == 0;
        h.overlay = v[WIND] ? GU_OVERLAY_WIND : GU_OVERLAY_NONE;
        h.overlay_param = v[GUST] ? 43691u : 0u;
        h.trail_cap = v[TRAIL] ? 8 : 0;
        h.entry_table_ok = v[ENTRY] != 0;
        for (int i = 0; i < COLUMNS - OPT0; ++i) h.opt[option[i]] = v[OPT0 + i];
        // (STRADDLE: some env passes a multiple of 2^32 steps during the launch -- which the launcher tells the plan of a policy that draws)
        const bool draws = v[POLICY] == GU_POLICY_UNIFORM || v[POLICY] == GU_POLICY_SAMPLE;
        const GuRolloutPlan p = gu_rollout_plan(&h, v[T], (int32_t)v[POLICY], (uint32_t)v[FLAGS], draws && v[STRADDLE] != 0, 0u);
        int32_t form[GU_FORM_WORDS];
        gu_rollout_plan_form(p, form);
        for (int i = 0; i < GU_FORM_WORDS; ++i) printf("%d%c", form[i], i + 1 < GU_FORM_WORDS ? ' ' : '\n');
    }
}
