// ioc_plane_pile.h — what k_ops_project_ins and k_plane_pile (ioc_plane_pile.hip) share with the host: the byte a slot plane holds,
// what a plane byte adds to a counter, the work item of k_plane_pile and where a wave leaves a counter in LDS.
// tools/plane_pile_check.cpp drives these on the CPU under the sanitizers, lane by lane, against the definitions
// (ioc_host_ops_project_ins, ioc_host_planes_pile).
#pragma once

#include <cstdint>

#include "ioc_ops_pileup.h"

#define IOC_PLANE_PILE_WAVES 4  // the waves of a workgroup of k_plane_pile: wave w takes the members w, w + 4, .. of its segment
#define IOC_PLANE_PILE_ROWS 64  // the rows of a work item: a lane per row

// 64 rows of a group-segment: group-segment gseg = 2 * segment + group, rows row .. row + 63 of it (those beyond rlen: idle lanes)
struct IocPlaneWork {
    uint32_t gseg, row;
};

// the byte of a slot plane for an inserted base of channel ch (0 .. 4): never 0, which says "nothing inserted"
IOC_PILE_HD uint32_t plane_slot_byte(uint32_t ch) { return 1u + ch; }
// a base-plane byte b adds to counter v (0 .. 5: a c g t other del) where it is v; IOC_ALLELE_NONE and any other byte add nothing
IOC_PILE_HD bool plane_base_adds(uint32_t b, uint32_t v) { return b == v; }
// a slot-plane byte s adds to channel ch (0 .. 4) of its slot where it is 1 + ch; 0 and any other byte add nothing
IOC_PILE_HD bool plane_slot_adds(uint32_t s, uint32_t ch) { return s == plane_slot_byte(ch); }
// counter k (0 .. 35: the six of the base plane, then slot-major five per slot) of a wave's share in LDS: counter-major, the
// lane added by the caller — 64 consecutive words per counter
IOC_PILE_HD uint32_t plane_part_at(uint32_t k) { return k * 64u; }
