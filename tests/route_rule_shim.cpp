// extern "C" wrappers around host/route_rule.h for tests/test_route_rule.py: plain C++17, no HIP
#include "../cuda-pathtracer_amd/host/route_rule.h"

#include <cstring>

using namespace ptmi;

extern "C" {

int shim_n_features() { return kRouteFeatures; }

static int put(const std::string& s, char* out, int cap) {
    if ((int)s.size() >= cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}
// the message's length (0: no refusal), the message in out; -1: out is too small
int shim_config_refusal(unsigned features, int integrator, int sampling_mode, int fast_tree, char* out, int cap) {
    return put(configRefusal(features, integrator, sampling_mode, fast_tree), out, cap);
}
int shim_feature_refusal(int feature, int integrator, int sampling_mode, int fast_tree, char* out, int cap) {
    return put(featureRefusal((RouteFeature)feature, integrator, sampling_mode, fast_tree), out, cap);
}
// bit 0: the per-lane route, bit 1: the lens and the medium blocks are handed over
int shim_route(unsigned features, int integrator) {
    const Route r = routeOf(features, integrator);
    return (r.per_lane ? 1 : 0) | (r.blocks ? 2 : 0);
}

}  // extern "C"
