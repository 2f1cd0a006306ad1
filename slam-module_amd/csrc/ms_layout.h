// ms_layout.h -- byte layout of the staging blocks of the map-side entry points (loop RANSAC, Sim3 optimise, project gate, map refresh /
// loop correct, covisibility / map point union, triangulate, observation count / map cull, observation lists, match tracked, map fuse, create points, BA window, search bind, loop chain, frame finish, keyframe admit, map extract, frame admit, map publish).  Plain C++17, no HIP: tests/ms_layout_check.cpp compiles it alone.
//
// A block is a run of arrays, each starting on a 256-byte boundary.  An entry point names every array once, in block order:
//     MsLayout up;                                          // upload block: rows | flags
//     const auto rows = up.array<int32_t>(n), flags = up.array<uint8_t>(n);
//     MsLayout host = up, dev = up;                         // the host block and the device block both start with the upload block ...
//     const auto down = host.array<int32_t>(n);             // ... and go on independently
//     const auto work = dev.array<double>(3 * n);
// and uses the name for the copy into the host block (rows.fill(hs, src)) and for the pointer a kernel gets (rows.at(ds)), so the element
// type and the count are written once.  `end` is the block's size so far.  (ba.hip's BaLayout is a different rule: it never takes less
// than 8 bytes.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

inline size_t ms_align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

template <class T> inline T *ms_at(void *base, size_t offset) { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + offset); }

// `count` elements of T at byte offset `off` of a block
template <class T> struct MsArray {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    T *at(void *base) const { return ms_at<T>(base, off); }
    // n elements into / out of the array from element `first` on (the caller keeps first + n <= count); nothing is touched for n = 0, so an
    // empty array may come with a null pointer
    void put(void *base, size_t first, const T *src, size_t n) const { if (n) std::memcpy(at(base) + first, src, n * sizeof(T)); }
    void get(void *base, size_t first, T *dst, size_t n) const { if (n) std::memcpy(dst, at(base) + first, n * sizeof(T)); }
    void fill(void *base, const T *src) const { put(base, 0, src, count); }                             // the whole array
};

struct MsLayout {
    static constexpr size_t kAlign = 256;
    size_t end = 0;
    // the offset of the next array; an array of no bytes shares it with the one after
    size_t take(size_t bytes) {
        const size_t at = end;
        end += ms_align_up(bytes, kAlign);
        return at;
    }
    template <class T> MsArray<T> array(size_t count) { return MsArray<T>{take(count * sizeof(T)), count}; }
};
