// Stand-alone check of Spawner::addRoutes (cityflow_amd/csrc/host/flow.cpp), the host side of Engine.add_routes: built with
// flow.cpp and roadnet.cpp by tests/test_add_routes_host.py (and by hand with -fsanitize=address,undefined) and run on a
// scenario's files.    add_routes_main <roadnet.json> <flow.json>    prints "ok"
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "flow.h"
#include "roadnet.h"

using cfa::HostRoadNet;
using cfa::Spawner;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static std::vector<int> roadsOf(const Spawner &s, int route) {
    const cfa::RouteTable &rt = s.routes;
    return std::vector<int>(rt.roads.begin() + rt.routeStart[(size_t) route], rt.roads.begin() + rt.routeStart[(size_t) route + 1]);
}

template <class F> static std::string thrown(F f) {
    try {
        f();
    } catch (const std::invalid_argument &e) {
        return e.what();
    }
    return "";
}

int main(int argc, char **argv) {
    if (argc != 3) return std::fprintf(stderr, "usage: %s roadnet.json flow.json\n", argv[0]), 2;
    HostRoadNet net;
    net.load(argv[1]);
    Spawner sp;
    sp.init(&net, 1.0, 1, 0);
    sp.loadFlows(argv[2]);
    const int n0 = sp.routes.count();
    EXPECT(n0 > 0);
    const std::vector<int> flow0 = roadsOf(sp, 0);
    EXPECT(flow0.size() >= 2);

    // a flow's own route dedupes onto its index; equal lists share one handle; nothing else is added
    std::vector<int> h = sp.addRoutes({flow0, flow0, {flow0.front(), flow0.back()}});
    EXPECT(h.size() == 3 && h[0] == 0 && h[1] == 0);
    EXPECT(roadsOf(sp, h[2]).front() == flow0.front() && roadsOf(sp, h[2]).back() == flow0.back());
    const int n1 = sp.routes.count();
    EXPECT(n1 == n0 + (h[2] >= n0 ? 1 : 0));
    EXPECT(sp.addRoutes({}).empty() && sp.routes.count() == n1);

    // every road to every other road: either a route (handle in range, first and last road as given) or refused as a whole
    const int R = (int) net.roads.size();
    int added = 0, refused = 0;
    for (int a = 0; a < R; ++a)
        for (int b = 0; b < R; ++b) {
            const int before = sp.routes.count();
            const std::string why = thrown([&] {
                const std::vector<int> got = sp.addRoutes({flow0, {a, b}});
                EXPECT(got.size() == 2 && got[0] == 0 && got[1] >= 0 && got[1] < sp.routes.count());
                const std::vector<int> roads = roadsOf(sp, got[1]);
                EXPECT(roads.size() >= 2 && roads.front() == a && roads.back() == b);
                ++added;
            });
            if (!why.empty()) {
                EXPECT(why.find("routes[1]") != std::string::npos && sp.routes.count() == before);
                ++refused;
            }
        }
    EXPECT(added > 0 && refused >= R);  // (a == b is a route of one road: refused)

    // bad road numbers, an empty list, one road: the index is named and nothing is added, not even the good lists before it
    const int n2 = sp.routes.count();
    EXPECT(thrown([&] { sp.addRoutes({flow0, {0, R}}); }).find("routes[1]") != std::string::npos);
    EXPECT(thrown([&] { sp.addRoutes({{-1, 0}}); }).find("routes[0]") != std::string::npos);
    EXPECT(thrown([&] { sp.addRoutes({flow0, flow0, {}}); }).find("routes[2]") != std::string::npos);
    EXPECT(thrown([&] { sp.addRoutes({{flow0[0]}}); }).find("routes[0]") != std::string::npos);
    EXPECT(sp.routes.count() == n2);

    // the tables stay a CSR over every route, and a reset drops none
    const cfa::RouteTable &rt = sp.routes;
    EXPECT(rt.routeStart.size() == (size_t) rt.count() + 1 && rt.routeStart.back() == (int32_t) rt.roads.size());
    EXPECT(rt.nextStart.size() == rt.roads.size() + 1 && rt.nextStart.back() == (int32_t) rt.nextLL.size());
    EXPECT(rt.firstLanes.size() == (size_t) rt.count());
    sp.reset(true);
    EXPECT(sp.routes.count() == n2 && sp.addRoutes({flow0})[0] == 0);

    if (failures) return 1;
    std::puts("ok");
    return 0;
}
