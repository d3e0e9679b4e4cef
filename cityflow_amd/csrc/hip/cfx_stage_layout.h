// The buffers of one C ABI call (plain C++17, no HIP: tests/tools/stage_layout_main.cpp builds it with the host compiler).
// A call that exists in a host form and a `_device` form (cfx_get_lane_obs / cfx_observe_lane_obs_device, cfx_set_tl_plan /
// cfx_set_tl_plan_device, ...) has ONE body in cfx_hip.hip, which declares the arrays it was given as fields, `in` or `out`,
// each with the name its error messages use, and launches on dev(field).  The layout's mode, fixed at construction, says what
// the caller's arrays are:
//   - staged (the host forms): host arrays.  Each field gets an offset into ONE device allocation, the engine's staging
//     arena (cfx_engine::stage), which copies the `in` fields up before the launch and the `out` fields back after it.
//       - Every offset is a multiple of kStageAlign.  (More than any kernel needs: they take element-aligned pointers.)
//       - A field whose host pointer is null takes no space and its device address is null: the kernels decide what to
//         compute by testing their output pointers.
//       - A field whose host pointer is NOT null gets a distinct device address inside the arena even with 0 bytes (an empty
//         network's outputs are still "given"), so size() is never 0 once a field is declared.
//   - pass-through (the `_device` forms): the caller's device buffers.  dev(field) is the caller's pointer, null for null;
//     no field takes arena space, and nothing is copied: the engine validates the pointers (cfx_engine::stageCheck) and orders
//     its stream against the caller's (stageOpen / stageClose).
// A field's element count may follow its declaration, any time before the engine opens the layout (count()): some calls know
// their row lengths only after preparing, and their `_device` forms validate the pointers before that.
#pragma once

#include <cstddef>
#include <cstdlib>

namespace cfx_stage {

constexpr size_t kStageAlign = 256;
constexpr int kStageMaxFields = 16;  // (cfx_observe_vehicles_device declares 15)

template <typename T> struct StageRef {  // a declared field, typed by what the device array holds
    int index;
};

struct StageLayout {
    struct Field {
        void *host;        // the caller's array (pass-through: the caller's device buffer); null: not given
        const char *name;  // what an error message calls it
        size_t bytes;
        bool out;          // copied back after the launch; otherwise copied up before it
        size_t offset;     // from the arena's base (meaningless where host is null, and in pass-through mode)
    };
    const bool passThrough;
    Field field[kStageMaxFields];
    int nFields = 0;
    size_t total = 0;      // arena bytes of the fields declared so far, a multiple of kStageAlign
    char *base = nullptr;  // the arena, once the engine has opened it for this layout

    explicit StageLayout(bool passThrough = false) : passThrough(passThrough) {}

    template <typename T> StageRef<const T> in(const T *host, const char *name, size_t count = 0) {
        return {add(const_cast<T *>(host), name, count * sizeof(T), false)};
    }
    template <typename T> StageRef<T> out(T *host, const char *name, size_t count = 0) {
        return {add(host, name, count * sizeof(T), true)};
    }
    // the element count of a field declared without one
    template <typename T> void count(StageRef<T> r, size_t n) {
        field[r.index].bytes = n * sizeof(T);
        place();
    }

    // what the arena has to hold (never 0: an opened arena is an allocation)
    size_t size() const { return total ? total : kStageAlign; }
    size_t offsetOf(int index) const { return field[index].offset; }
    template <typename T> T *dev(StageRef<T> r) const {
        const Field &f = field[r.index];
        return passThrough ? (T *) f.host : f.host ? (T *) (base + f.offset) : nullptr;
    }

private:
    int add(void *host, const char *name, size_t bytes, bool out) {
        if (nFields == kStageMaxFields) std::abort();  // (a call with more arrays raises the constant)
        field[nFields++] = Field{host, name, bytes, out, 0};
        place();
        return nFields - 1;
    }
    void place() {
        total = 0;
        for (int i = 0; i < nFields; ++i) {
            Field &f = field[i];
            f.offset = total;
            if (f.host && !passThrough) total += ((f.bytes ? f.bytes : 1) + kStageAlign - 1) / kStageAlign * kStageAlign;
        }
    }
};

}  // namespace cfx_stage
