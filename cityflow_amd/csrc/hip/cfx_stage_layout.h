// The bookkeeping of one staged call (plain C++17, no HIP: tests/tools/stage_layout_main.cpp builds it with the host
// compiler).  A host form of the C ABI (cfx_get_lane_obs, cfx_set_tl_plan, ...) declares the host arrays it was given as
// fields, `in` or `out`; each field gets an offset into ONE device allocation, the engine's staging arena (cfx_engine::stage,
// cfx_hip.hip), which copies the `in` fields up before the launch and the `out` fields back after it.
//   - Every offset is a multiple of kStageAlign.  (More than any kernel needs: they take element-aligned pointers.)
//   - A field whose host pointer is null takes no space and its device address is null: the kernels decide what to compute by
//     testing their output pointers.
//   - A field whose host pointer is NOT null gets a distinct device address inside the arena even with 0 bytes (an empty
//     network's outputs are still "given"), so size() is never 0 once a field is declared.
#pragma once

#include <cstddef>
#include <cstdlib>

namespace cfx_stage {

constexpr size_t kStageAlign = 256;
constexpr int kStageMaxFields = 12;  // (the lane observations declare 9)

template <typename T> struct StageRef {  // a declared field, typed by what the device array holds
    int index;
};

struct StageLayout {
    struct Field {
        void *host;     // the caller's array; null: not given
        size_t bytes;
        bool out;       // copied back after the launch; otherwise copied up before it
        size_t offset;  // from the arena's base (meaningless where host is null)
    };
    Field field[kStageMaxFields];
    int nFields = 0;
    size_t total = 0;      // bytes of the fields declared so far, a multiple of kStageAlign
    char *base = nullptr;  // the arena, once the engine has opened it for this layout

    template <typename T> StageRef<const T> in(const T *host, size_t count) {
        return {add(const_cast<T *>(host), count * sizeof(T), false)};
    }
    template <typename T> StageRef<T> out(T *host, size_t count) { return {add(host, count * sizeof(T), true)}; }

    // what the arena has to hold (never 0: an opened arena is an allocation)
    size_t size() const { return total ? total : kStageAlign; }
    size_t offsetOf(int index) const { return field[index].offset; }
    template <typename T> T *dev(StageRef<T> r) const {
        return field[r.index].host ? (T *) (base + field[r.index].offset) : nullptr;
    }

private:
    int add(void *host, size_t bytes, bool out) {
        if (nFields == kStageMaxFields) std::abort();  // (a form with more arrays raises the constant)
        field[nFields] = Field{host, bytes, out, total};
        if (host) total += ((bytes ? bytes : 1) + kStageAlign - 1) / kStageAlign * kStageAlign;
        return nFields++;
    }
};

}  // namespace cfx_stage
