// extern "C" wrappers around host/launch_rule.h for tests/test_launch_rule.py: plain C++17, no HIP
#include "../cuda-pathtracer_amd/host/launch_rule.h"

using namespace ptmi;

extern "C" {

// walk: 0 lane / stack, 1 phased / packed, 2 sweep, 3 wide / certified
struct shim_rule_in {
    int walk, segments_per_launch, spp;
    long long n_local;
    int n_frames, nee, is_pass, want_chunks;
    long long wave_slots;
    int use_env;                                     // 1: the overrides come from the environment (LaunchOverrides::fromEnv)
};
struct shim_rule_out {
    int needs_wave_slots, segments, rest_segments;
    long long fit_pct;
    int refill, run_ahead, order_by_cost, order_classes, auto_chunks, publish;
};

static LaunchWalk walk_of(int walk) {
    LaunchWalk w;
    w.phased = walk == 1 || walk == 3; w.wide = walk == 3; w.sweep = walk == 2;
    return w;
}
static LaunchRule plan_of(const shim_rule_in* in, LaunchOverrides* over_out) {
    LaunchRuleInput i;
    i.walk = walk_of(in->walk);
    i.segments_per_launch = in->segments_per_launch; i.spp = in->spp; i.n_local = in->n_local; i.n_frames = in->n_frames;
    i.nee = in->nee != 0; i.is_pass = in->is_pass != 0; i.want_chunks = in->want_chunks; i.wave_slots = in->wave_slots;
    if (in->use_env) i.over = LaunchOverrides::fromEnv();
    if (over_out) *over_out = i.over;
    return LaunchRule::plan(i);
}

void shim_plan(const shim_rule_in* in, shim_rule_out* out) {
    LaunchOverrides over;
    const LaunchRule p = plan_of(in, &over);
    out->needs_wave_slots = LaunchRule::needsWaveSlots(walk_of(in->walk), in->segments_per_launch) ? 1 : 0;
    out->segments = p.segments; out->rest_segments = p.rest_segments; out->fit_pct = p.fit_pct;
    out->refill = p.refill ? 1 : 0; out->run_ahead = p.run_ahead;
    out->order_by_cost = p.order_by_cost ? 1 : 0; out->order_classes = p.order_classes; out->auto_chunks = p.auto_chunks;
    out->publish = over.publish ? 1 : 0;
}
// per launch: out4 = fits, many_waves, max_waves, segments of the launch
void shim_launch(const shim_rule_in* in, long long active, long long bound, int* out4) {
    const LaunchRule p = plan_of(in, nullptr);
    out4[0] = p.fits(active) ? 1 : 0; out4[1] = p.manyWaves(active) ? 1 : 0; out4[2] = p.maxWaves(active, bound); out4[3] = p.launchSegments(active);
}
int shim_cost_order(const shim_rule_in* in, int n_chunks) { return plan_of(in, nullptr).costOrder(n_chunks) ? 1 : 0; }

}  // extern "C"
