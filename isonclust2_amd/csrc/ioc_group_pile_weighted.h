// ioc_group_pile_weighted.h — what k_ops_project_weights and k_group_pile_weighted (ioc_group_pile_weighted.hip) share with the
// host: the layout of the seven weight planes, the counters a lane of the pile keeps and where a wave leaves them in LDS, and what
// a plane byte adds to a count or to a sum of weights.  The work item, the waves of a workgroup, the members in flight, the steps
// known ahead and which positions of a member list a wave takes are those of k_group_pile (ioc_group_pile.h), whose shape this
// kernel has.  tools/group_pile_weighted_check.cpp drives these on the CPU under the sanitizers, lane by lane, against the
// definitions (ioc_host_ops_project_weights, ioc_host_planes_pile and ioc_host_planes_pile_weighted over every group's reads).
#pragma once

#include <cstdint>

#include "ioc_group_pile.h"
#include "isonclust2_hip.h"

#define IOC_WEIGHT_PLANES (1 + IOC_PILE_INS_SLOTS)  // [wbase plane][wslot-0 planes] .. [wslot-5 planes], plane_bytes each

// The counters of a lane, in the order they lie in LDS: the six counts of gcols, ins_runs, ins_bases, the six sums of gwcols, the
// thirty sums of gwins (slot-major, five per slot).
enum : uint32_t {
    GPW_COUNT = 0,                                      // a c g t other del: how many reads say so
    GPW_RUNS = 6,                                       // slot-0 bytes that insert
    GPW_BASES = 7,                                      // slot bytes that insert
    GPW_WBASE = 8,                                      // a c g t other del: the sum of their weights
    GPW_WSLOT = 14,                                     // slot j, channel ch at GPW_WSLOT + 5 j + ch: the sum of the weights
    GPW_ACC = GPW_WSLOT + 5u * IOC_PILE_INS_SLOTS       // 44
};
static_assert(GPW_ACC == 44u, "six counts, two insertion counts, six and thirty sums of weights");

// the plane (0 .. 6) of the weight of a base-plane byte / of a byte of slot plane j: a pair's bytes of plane k lie at
// k * plane_bytes + its `plane` offset, as its base and slot bytes do in their planes
IOC_PILE_HD uint32_t weight_plane_base() { return 0u; }
IOC_PILE_HD uint32_t weight_plane_slot(uint32_t j) { return 1u + j; }
// a slot-plane byte inserts where it is one of 1 .. 5 (plane_slot_byte of a channel); 0 and any other byte insert nothing
IOC_PILE_HD bool plane_slot_inserts(uint32_t s) { return s - 1u < 5u; }
// what a base-plane byte b with weight byte w adds to the sum of counter v (0 .. 5), and a slot byte s with weight w to channel ch
IOC_PILE_HD uint32_t plane_base_weighs(uint32_t b, uint32_t w, uint32_t v) { return plane_base_adds(b, v) ? w : 0u; }
IOC_PILE_HD uint32_t plane_slot_weighs(uint32_t s, uint32_t w, uint32_t ch) { return plane_slot_adds(s, ch) ? w : 0u; }
// the words a workgroup keeps in LDS: the counters of the waves 1 .. IOC_GROUP_PILE_WAVES - 1, counter-major (plane_part_at)
IOC_PILE_HD uint32_t group_pile_weighted_lds_words() { return (IOC_GROUP_PILE_WAVES - 1u) * GPW_ACC * 64u; }
