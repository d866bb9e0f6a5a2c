// ioc_group_pile.h — what k_group_pile (ioc_group_pile.hip) shares with the host: its work item, the waves of a workgroup, how
// many members a wave keeps in flight and how many steps ahead it knows where their planes lie, which positions of a group's
// member list a wave takes, and the byte a lane holds where it has nothing to read.  What a plane byte adds to a counter and
// where a wave leaves a counter in LDS are those of k_plane_pile (ioc_plane_pile.h).  tools/group_pile_check.cpp drives these on
// the CPU under the sanitizers, lane by lane, against the definition (ioc_host_planes_pile over every group's reads).
#pragma once

#include <cstdint>

#include "ioc_plane_pile.h"

#define IOC_GROUP_PILE_WAVES 4   // the waves of a workgroup: wave w takes the positions w, w + 4, .. of its group's member list
#define IOC_GROUP_PILE_FLIGHT 2  // the members a wave has in flight: the planes of the next one are read before the current one's are added
#define IOC_GROUP_PILE_AHEAD 64  // the steps of a wave whose plane offsets it holds at a time, lane l that of step l of the chunk
#define IOC_GROUP_PILE_ROWS 64   // the rows of a work item: a lane per row

// 64 rows of a group-segment: group-segment gseg (segment order, gseg_off[g] + h), rows row .. row + 63 of it (those beyond rlen: idle lanes)
struct IocGroupWork {
    uint32_t gseg, row;
};

// the position of a group's member list that wave w reads in its step t (0, 1, ..), from the list's first position m0 on
IOC_PILE_HD uint32_t group_pile_at(uint32_t m0, uint32_t w, uint32_t t) { return m0 + w + t * IOC_GROUP_PILE_WAVES; }
// what a lane holds of a base plane where it reads nothing (an idle lane, a row outside the planes, a step behind the list): a
// byte that adds to no counter (plane_base_adds); of a slot plane it holds 0, which adds to none either (plane_slot_adds)
IOC_PILE_HD uint32_t group_pile_no_base() { return 0xFFu; }
// the steps wave w has over the positions m0 .. m1 - 1 of a list, and the plane offset a lane holds for a step that reads nothing
IOC_PILE_HD uint32_t group_pile_steps(uint32_t m0, uint32_t m1, uint32_t w)
{
    return m0 + w < m1 ? (m1 - (m0 + w) + IOC_GROUP_PILE_WAVES - 1u) / IOC_GROUP_PILE_WAVES : 0u;
}
IOC_PILE_HD uint64_t group_pile_no_plane() { return ~uint64_t(0); }
