// ssf_stage_layout.hpp -- where the items of one call sit in the staging buffer that carries host arrays through the device
// (StagedIo, ssf_handle.hpp).  Only the arithmetic, and no HIP header: tests/cpp/stage_layout_smoke.cpp runs it on the CPU.
#pragma once
#include <cstddef>

namespace ssf {

// Items in the order they were added.  An item with a host array starts on a multiple of 256 bytes behind the one before it; an
// item without one (a NULL output) takes no space.  total = the bytes the buffer needs.
struct StageLayout {
    enum { MAX_ITEMS = 24 };                                      // (the rollouts with movers declare 21)
    struct Item { const void* host; size_t bytes, off; };
    Item item[MAX_ITEMS];
    int n = 0;
    size_t total = 0;
    static size_t align(size_t b) { return (b + 255) & ~(size_t)255; }
    // returns the item's number, or -1 when the layout is full
    int add(const void* host, size_t bytes) {
        if (n == MAX_ITEMS) return -1;
        item[n] = Item{host, bytes, total};
        if (host) total += align(bytes);
        return n++;
    }
    // item i's place in a buffer that starts at base: nullptr for an item without a host array
    unsigned char* at(unsigned char* base, int i) const { return item[i].host ? base + item[i].off : nullptr; }
};

}  // namespace ssf
