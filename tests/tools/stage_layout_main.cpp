// Stand-alone check of csrc/hip/cfx_stage_layout.h (tests/test_stage_layout.py builds and runs it): fields are declared the
// way the host forms of cfx_hip.hip declare theirs, against a fake arena base, and every layout is held against the header's
// rules.  Prints "ok" and returns 0, or the first violated rule and 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cfx_stage_layout.h"

using namespace cfx_stage;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (failures++ < 20) {            \
                printf("FAILED %s: ", #cond); \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

struct Decl {
    bool given;
    size_t bytes;
    bool out;
};

alignas(256) static char arena[1 << 20];  // (never touched: the layout only computes addresses)
static char hostArray[8];                 // what a given field's host pointer points at

// declares `decl` in this order and checks the layout; returns its size
static size_t checkLayout(const char *name, const std::vector<Decl> &decl) {
    StageLayout s;
    std::vector<StageRef<char>> ref;
    for (const Decl &d : decl) {
        char *host = d.given ? hostArray : nullptr;
        ref.push_back(d.out ? s.out(host, "f", d.bytes) : StageRef<char>{s.in((const char *) host, "f", d.bytes).index});
    }
    s.base = arena;
    CHECK(s.nFields == (int) decl.size(), "%s: %d fields", name, s.nFields);
    CHECK(s.size() > 0 && s.size() % kStageAlign == 0, "%s: size %zu", name, s.size());
    CHECK(s.size() <= sizeof arena, "%s: size %zu beyond the test's arena", name, s.size());
    size_t sum = 0;
    for (size_t i = 0; i < decl.size(); ++i) {
        const StageLayout::Field &f = s.field[i];
        char *dev = s.dev(ref[i]);
        CHECK(f.out == decl[i].out && f.bytes == decl[i].bytes, "%s: field %zu is not what was declared", name, i);
        if (!decl[i].given) {
            CHECK(dev == nullptr, "%s: field %zu has no host pointer and a device address", name, i);
            continue;
        }
        sum += decl[i].bytes;
        CHECK(dev != nullptr, "%s: field %zu has a host pointer and no device address", name, i);
        CHECK(dev == arena + s.offsetOf((int) i), "%s: field %zu is not at its offset", name, i);
        CHECK(f.offset % kStageAlign == 0, "%s: field %zu at offset %zu", name, i, f.offset);
        // inside the arena, one byte at least even where it holds none
        const size_t end = f.offset + (f.bytes ? f.bytes : 1);
        CHECK(end <= s.size(), "%s: field %zu ends at %zu of %zu", name, i, end, s.size());
        for (size_t j = 0; j < i; ++j) {
            if (!decl[j].given) continue;
            const StageLayout::Field &g = s.field[j];
            const size_t gEnd = g.offset + (g.bytes ? g.bytes : 1);
            CHECK(end <= g.offset || gEnd <= f.offset, "%s: fields %zu and %zu overlap", name, j, i);
            CHECK(s.dev(ref[j]) != dev, "%s: fields %zu and %zu share an address", name, j, i);
        }
    }
    CHECK(s.size() >= sum, "%s: size %zu below the fields' %zu bytes", name, s.size(), sum);
    // null fields take no space: the same declarations without them give the same size
    std::vector<Decl> givenOnly;
    for (const Decl &d : decl)
        if (d.given) givenOnly.push_back(d);
    if (givenOnly.size() != decl.size()) {
        StageLayout t;
        for (const Decl &d : givenOnly) d.out ? (void) t.out(hostArray, "f", d.bytes) : (void) t.in((const char *) hostArray, "f", d.bytes);
        CHECK(t.size() == s.size(), "%s: %zu bytes with the null fields, %zu without", name, s.size(), t.size());
    }
    return s.size();
}

int main() {
    // nothing declared, and nothing given: still an allocation's worth
    CHECK(checkLayout("empty", {}) == kStageAlign, "empty");
    CHECK(checkLayout("all null", {{false, 4000, true}, {false, 0, false}}) == kStageAlign, "all null");
    // one field of every size around the alignment
    for (size_t bytes : {(size_t) 0, (size_t) 1, (size_t) 4, (size_t) 255, (size_t) 256, (size_t) 257, (size_t) 511, (size_t) 512,
                         (size_t) 4097})
        checkLayout("one field", {{true, bytes, true}});
    // zero bytes with a host pointer (an empty network's outputs): distinct addresses, also next to each other and last
    checkLayout("zero bytes", {{true, 0, true}, {true, 0, true}, {true, 0, false}});
    checkLayout("zero between", {{true, 100, true}, {true, 0, true}, {true, 100, true}, {true, 0, false}});
    // the shapes of the host forms: lane observations (8 outputs, the edges in), a plan (3 in), speed commands (2 in, 1 out)
    const std::vector<Decl> laneObs = {{true, 4 * 1001, true}, {true, 4 * 1001, true}, {false, 8 * 1001, true}, {true, 4 * 1001 * 32, true},
                                       {true, 8 * 1001 * 3, true}, {false, 8 * 1001 * 3, true}, {true, 4 * 1001 * 3, true},
                                       {false, 4 * 1001 * 3, true}, {true, 8 * 33, false}};
    const size_t laneObsSize = checkLayout("lane observations", laneObs);
    checkLayout("plan", {{true, 8 * 9 * 8, false}, {false, 4 * 9, false}, {true, 8 * 9, false}});
    checkLayout("speed commands", {{true, 4 * 777, false}, {true, 8 * 777, false}, {true, 4, true}});
    // another order of declaration: a valid layout again, of the same size
    {
        std::vector<Decl> reversed(laneObs.rbegin(), laneObs.rend());
        CHECK(checkLayout("lane observations, reversed", reversed) == laneObsSize, "reversed: another size");
        std::vector<Decl> rotated(laneObs.begin() + 4, laneObs.end());
        rotated.insert(rotated.end(), laneObs.begin(), laneObs.begin() + 4);
        CHECK(checkLayout("lane observations, rotated", rotated) == laneObsSize, "rotated: another size");
    }
    // as many fields as the list holds
    checkLayout("full", std::vector<Decl>((size_t) kStageMaxFields, Decl{true, 300, true}));
    // typed fields: the element count times the element's size
    {
        StageLayout s;
        double d[3];
        int32_t w[5];
        const auto fD = s.out(d, "d", 3);
        const auto fW = s.in((const int32_t *) w, "w", 5);
        s.base = arena;
        CHECK(s.field[fD.index].bytes == 24 && s.field[fW.index].bytes == 20, "typed fields: %zu and %zu bytes",
              s.field[fD.index].bytes, s.field[fW.index].bytes);
        CHECK((char *) s.dev(fD) == arena && (const char *) s.dev(fW) == arena + kStageAlign, "typed fields: addresses");
        CHECK(s.field[fD.index].out && !s.field[fW.index].out && s.field[fD.index].host == d && s.field[fW.index].host == w,
              "typed fields: direction and host pointer");
    }
    // every field keeps the name it was declared with
    {
        StageLayout s;
        const auto fA = s.out(hostArray, "left_waiting_steps", 8);
        const auto fB = s.in((const char *) nullptr, "edges", 8);
        CHECK(!s.passThrough, "a default layout is staged");
        CHECK(!strcmp(s.field[fA.index].name, "left_waiting_steps") && !strcmp(s.field[fB.index].name, "edges"), "staged: names");
    }
    // pass-through (the `_device` forms): the caller's pointers come back as they are, null for null, whatever the counts;
    // no field takes arena space; names per field; as many fields as the list holds (cfx_observe_vehicles_device: 15)
    {
        static const char *const names[16] = {"f0", "f1", "f2", "f3", "f4", "f5", "f6", "f7", "f8", "f9", "f10", "f11", "f12", "f13", "f14", "f15"};
        static_assert(kStageMaxFields >= 16, "cfx_observe_vehicles_device declares 15 buffers");
        static double buffer[16][3];
        StageLayout s(true);
        CHECK(s.passThrough, "pass-through: the mode");
        StageRef<double> out[16];
        StageRef<const double> in[16];
        for (int i = 0; i < 16; ++i) {
            double *p = i % 5 == 3 ? nullptr : &buffer[i][i % 3];  // (some null, none aligned to anything but its type)
            const size_t count = i % 4 == 0 ? 0 : (size_t) 1000 * i;
            if (i % 2) in[i] = s.in((const double *) p, names[i], count);
            else out[i] = s.out(p, names[i], count);
        }
        s.base = arena;  // (an engine never sets it for this mode; it must not matter)
        CHECK(s.nFields == 16, "pass-through: %d fields", s.nFields);
        CHECK(s.size() == kStageAlign, "pass-through: fields take %zu bytes of the arena", s.size());
        for (int i = 0; i < 16; ++i) {
            const double *p = i % 5 == 3 ? nullptr : &buffer[i][i % 3];
            const double *dev = i % 2 ? s.dev(in[i]) : s.dev(out[i]);
            CHECK(dev == p, "pass-through: field %d is not the caller's pointer", i);
            CHECK(!strcmp(s.field[i].name, names[i]), "pass-through: field %d is called %s", i, s.field[i].name);
        }
        // a count that follows changes neither
        s.count(out[0], 12345);
        CHECK(s.size() == kStageAlign && s.dev(out[0]) == &buffer[0][0], "pass-through: a late count moved something");
    }
    // late counts: a count given after the declaration (any time before the open, in any order) gives the layout that the same
    // count gives at the declaration
    {
        double d[4];
        int32_t w[4];
        const size_t counts[4] = {1001, 0, 33, 700};
        StageLayout early, late;
        const auto e0 = early.out(d, "a", counts[0]), e1 = early.out(d + 1, "b", counts[1]);
        const auto e2 = early.in((const int32_t *) w, "c", counts[2]);
        const auto e3 = early.out((double *) nullptr, "d", counts[3]);
        const auto l0 = late.out(d, "a"), l1 = late.out(d + 1, "b");
        const auto l2 = late.in((const int32_t *) w, "c");
        const auto l3 = late.out((double *) nullptr, "d");
        late.count(l2, counts[2]), late.count(l3, counts[3]), late.count(l0, counts[0]), late.count(l1, counts[1]);
        early.base = late.base = arena;
        CHECK(early.size() == late.size(), "late counts: %zu bytes, %zu with the counts at the declaration", late.size(), early.size());
        for (int i = 0; i < 4; ++i) {
            const StageLayout::Field &a = early.field[i], &b = late.field[i];
            CHECK(a.host == b.host && a.bytes == b.bytes && a.out == b.out && a.offset == b.offset && !strcmp(a.name, b.name),
                  "late counts: field %d differs (%zu bytes at %zu, %zu at %zu)", i, b.bytes, b.offset, a.bytes, a.offset);
        }
        CHECK(early.dev(e0) == late.dev(l0) && early.dev(e1) == late.dev(l1) && early.dev(e2) == late.dev(l2) &&
                  early.dev(e3) == late.dev(l3) && late.dev(l3) == nullptr,
              "late counts: device addresses");
        CHECK(late.dev(l1) != late.dev(l0) && (char *) late.dev(l1) == arena + late.offsetOf(1), "late counts: the empty field's address");
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
