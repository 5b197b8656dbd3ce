// route_rule_check.cpp — a stand-alone caller of host/route_rule.h, to be built with -fsanitize=address,undefined
// (tests/test_route_rule.py): every feature mask x config in the config direction and for the route, every settable feature x
// config in the setter direction.  Each answer is held against the rule restated here: which (feature, field) pair answers, and
// that the message is made of that pair's parts.  The exact words are tests/test_route_rule.py's business.
#include "../cuda-pathtracer_amd/host/route_rule.h"

#include <cstdio>

using namespace ptmi;

static int cases = 0, failed = 0;
static void check(bool ok, const char* what, unsigned a, int i, int m, int t) {
    cases++;
    if (!ok) { failed++; std::printf("FAILED %s: features/feature %u, integrator %d, sampling_mode %d, fast_tree %d\n", what, a, i, m, t); }
}
// all but the lens and the medium refuse integrator 1; every feature refuses a guided mode and the fast tree
static bool refuses(int f, int field) { return field != kRouteIntegrator || (f != kRouteLens && f != kRouteMedium); }
static bool begins(const std::string& s, const std::string& with) { return s.compare(0, with.size(), with) == 0; }
static bool ends(const std::string& s, const std::string& with) { return s.size() >= with.size() && s.compare(s.size() - with.size(), with.size(), with) == 0; }

// the message of (f, field) in one direction is made of the row's parts, or empty where there is no such pair
static bool wellFormed(const std::string& msg, int f, int field, bool to_config) {
    if (f < 0) return msg.empty();
    const RouteRow& r = kRouteRows[f];
    const char* why = field == kRouteFastTree ? r.why_fast : to_config ? r.why_config[field] : r.why_setter[field];
    if (!why) return false;
    if (to_config) return begins(msg, std::string(r.is_set) + " " + kNeeds[field] + ": ") && ends(msg, why);
    return begins(msg, std::string(r.setter) + ": the config has " + kHas[field]) && ends(msg, why);
}

int main() {
    for (int integrator = 0; integrator < 2; integrator++)
        for (int mode = 0; mode < 5; mode++)
            for (int fast = 0; fast < 2; fast++) {
                const bool offends[kRouteFields] = {integrator != 0, mode != 0, fast != 0};
                for (unsigned mask = 0; mask < 1u << kRouteFeatures; mask++) {
                    int f_first = -1, k_first = -1;
                    for (int f = kRouteFeatures - 1; f >= 0; f--)
                        for (int k = kRouteFields - 1; k >= 0; k--)
                            if ((mask >> f & 1) && offends[k] && refuses(f, k)) { f_first = f; k_first = k; }
                    const Route route = routeOf(mask, integrator);
                    check(wellFormed(configRefusal(mask, integrator, mode, fast), f_first, k_first, true) &&
                              route.per_lane == (mask != 0 && integrator == 0) && route.blocks == (integrator == 0),
                          "config direction / route", mask, integrator, mode, fast);
                }
                for (int f = kRouteEnvironment; f < kRouteFeatures; f++) {
                    int k_first = -1;
                    for (int k = kRouteFields - 1; k >= 0; k--) if (offends[k] && refuses(f, k)) k_first = k;
                    check(wellFormed(featureRefusal((RouteFeature)f, integrator, mode, fast), k_first < 0 ? -1 : f, k_first, false),
                          "setter direction", (unsigned)f, integrator, mode, fast);
                }
            }
    std::printf("%s %d\n", failed ? "failed" : "ok", failed ? failed : cases);
    return failed ? 1 : 0;
}
