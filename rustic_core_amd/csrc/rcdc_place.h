// rcdc_place_blobs: what the host half (rcdc_place.cpp, its tile planner in
// rcdc_family_plans.h) and the kernel (rcdc_place.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rcdc {

// One tile: at most kPlaceTile source bytes of one blob, one workgroup's work.
// src is the device address of the tile's first byte; the tile goes to
// daddr[dest0 + d] + off for d < ndests (daddr: the device address of each
// destination's first byte).  kPlaceAligned in off: every destination is
// congruent to the source mod 16, so no lane needs its neighbour's granule.
struct PlaceTile {
    uint64_t src;
    uint32_t len, blob;
    uint32_t dest0, ndests;
    uint64_t off;
};
static_assert(sizeof(PlaceTile) == 32, "PlaceTile is 32 B");

constexpr uint32_t kPlaceTile = 64u << 10;
constexpr uint64_t kPlaceAligned = 1ull << 63;

// write: copy to the destinations; zero: OR the tile's bytes into nz[blob];
// skip (with write): leave out the blobs whose nz word is still 0.
hipError_t launch_place(const PlaceTile *tiles, uint32_t n, const uint64_t *daddr, uint32_t *nz,
                        bool write, bool zero, bool skip, uint32_t cus, hipStream_t stream);

}  // namespace rcdc
