// ioc_ops_pileup.h — the step logic of k_ops_pileup (ioc_ops_pileup.hip), callable on the host as well: tools/pileup_acc_check.cpp
// drives it over strings on the CPU, under the sanitizers, against the definition (ioc_host_ops_pileup), tools/pile_weight_check.cpp
// the weights of the weighted variant against ioc_host_ops_pileup_weighted.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define IOC_PILE_HD __host__ __device__ inline __attribute__((always_inline))  // (__forceinline__, also where no HIP header came first)
#else
#define IOC_PILE_HD inline
#endif

// the channels of a row as words of ioc_pileup_col
enum : uint32_t { PILE_A = 0, PILE_C, PILE_G, PILE_T, PILE_OTHER, PILE_DEL, PILE_INS_RUNS, PILE_INS_BASES, PILE_WORDS };

// the weight of a quality byte in the weighted pileup (ioc_host_qual_weight): 1 .. 93, never 0
IOC_PILE_HD uint32_t pile_qual_weight(uint8_t b) { return b <= 34u ? 1u : b - 33u < 93u ? b - 33u : 93u; }

// Where a wave stands in its string; one step per 64 bytes, bit l of a mask = the l-th of them (bytes outside the string are 0
// in every mask).  The members are the same in every lane (the masks are ballots); what differs per lane is the argument l.
struct PileAcc {
    uint32_t r = 0, q = 0;  // reference / query bases consumed before this step
    bool open_i = false;    // the byte before this step is 'I'
    uint32_t open_len = 0;  // (the ins variant, end_len) ... and the 'I's that end there: open_i is open_len != 0
    unsigned long long m_ref = 0, m_qry = 0, m_base = 0, m_del = 0, m_ins = 0;

    IOC_PILE_HD void begin(unsigned long long m_eq, unsigned long long m_x, unsigned long long m_i, unsigned long long m_d,
                           unsigned long long e_i, unsigned long long e_d)
    {
        m_base = m_eq | m_x;
        m_del = m_d;
        m_ins = m_i;
        m_ref = m_base | m_d | e_d;
        m_qry = m_base | m_i | e_i;
    }
    static IOC_PILE_HD unsigned long long below(uint32_t l) { return (1ull << l) - 1ull; }
    // the reference position lane l's byte stands at (in front of, for an 'I'), and the query base it takes
    IOC_PILE_HD uint32_t row(uint32_t l) const { return r + uint32_t(__builtin_popcountll(m_ref & below(l))); }
    IOC_PILE_HD uint32_t qpos(uint32_t l) const { return q + uint32_t(__builtin_popcountll(m_qry & below(l))); }
    IOC_PILE_HD bool is_base(uint32_t l) const { return (m_base >> l) & 1ull; }
    IOC_PILE_HD bool is_del(uint32_t l) const { return (m_del >> l) & 1ull; }
    // (the weighted variant) the weight of a 'D' lane: the smaller of the weights of the query bases on its two sides, q - 1 and
    // q of the qlen bases whose quality bytes stand at `qual`, where they exist; 1 where neither does
    IOC_PILE_HD uint32_t del_weight(uint32_t l, uint32_t qlen, const uint8_t* qual) const
    {
        const uint32_t at = qpos(l);
        const uint32_t a = at > 0u && at - 1u < qlen ? pile_qual_weight(qual[at - 1u]) : 0u;
        const uint32_t b = at < qlen ? pile_qual_weight(qual[at]) : 0u;
        return a == 0u ? (b == 0u ? 1u : b) : b == 0u || a < b ? a : b;
    }
    // The 'I' bytes of a step are added piece by piece — a piece: consecutive 'I's within the step, all in front of one row — by
    // the lane of the piece's first byte: its length, 0 for every other lane.  One add per piece, not one per byte on one address.
    IOC_PILE_HD uint32_t ins_piece(uint32_t l) const
    {
        if (!(((m_ins & ~(m_ins << 1)) >> l) & 1ull)) return 0u;
        const unsigned long long x = ~(m_ins >> l);  // (0 only for l == 0 under a mask of all ones)
        return x ? uint32_t(__builtin_ctzll(x)) : 64u;
    }
    // a maximal run of 'I' starts at lane l: the piece's first lane, unless the run came in from the step before
    IOC_PILE_HD bool run_start(uint32_t l) const { return ((m_ins & ~((m_ins << 1) | (open_i ? 1ull : 0ull))) >> l) & 1ull; }
    // (the ins variant) the index of lane l's 'I' within its maximal run: the 'I's directly below the lane, and the run's length
    // before this step where they reach down to the step's first byte
    IOC_PILE_HD bool is_ins(uint32_t l) const { return (m_ins >> l) & 1ull; }
    IOC_PILE_HD uint32_t ins_index(uint32_t l) const
    {
        const unsigned long long t = ~m_ins & below(l);  // the bytes below the lane that are no 'I'
        return t ? l - (64u - uint32_t(__builtin_clzll(t))) : l + open_len;
    }
    // (the ins variant) called in front of end(): carries the length of a run that reaches the step's last byte
    IOC_PILE_HD void end_len()
    {
        const unsigned long long t = ~m_ins;
        open_len = t ? uint32_t(__builtin_clzll(t)) : open_len + 64u;  // (the ones at the top of m_ins)
    }
    IOC_PILE_HD void end()
    {
        r += uint32_t(__builtin_popcountll(m_ref));
        q += uint32_t(__builtin_popcountll(m_qry));
        open_i = (m_ins >> 63) != 0ull;
    }
    static IOC_PILE_HD uint32_t channel(uint8_t base)
    {
        return base == uint8_t('A') ? PILE_A : base == uint8_t('C') ? PILE_C : base == uint8_t('G') ? PILE_G : base == uint8_t('T') ? PILE_T : PILE_OTHER;
    }
};
