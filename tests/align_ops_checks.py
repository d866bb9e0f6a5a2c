"""What an operation string ('=' 'X' 'I' 'D', free end gaps 'i' 'd': ioc_host_align_ops, ioc_align_pairs_ops) must satisfy by
itself, whoever produced it — shared by tests/test_align_ops_host.py and tests/test_gpu_align_ops.py."""
import re

_COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def revcomp(s):
    return bytes(_COMP.get(ch, ch) for ch in reversed(s))


def check_ops(ops, q, r, score, gap_open, match=2, mismatch=-2, gap_extend=1, tag=None, any_gap_costs=False):
    """Checks 1 - 4 of an operation string against its two sequences (r already reverse-complemented where the pair asks for it)
    and the score reported with it.  Check 4 with gap_open > gap_extend: the DP then never puts two separate gaps of one kind
    side by side (one gap of length a + b is cheaper), so every maximal run of 'I' or of 'D' is ONE gap.  A caller that means to
    pass gap_open <= gap_extend says so (any_gap_costs): a run of length L is then as many gaps as is cheapest — every column a
    gap of its own where opening costs less than extending — and re-scores to gap_open + (L - 1) min(gap_open, gap_extend)."""
    assert gap_open > gap_extend or any_gap_costs
    run_step = gap_extend if gap_open > gap_extend else min(gap_open, gap_extend)  # what a run's second and later columns cost
    # 1. every base of either sequence in exactly one column
    assert sum(ops.count(c) for c in b"=XIi") == len(q), (tag, "query length")
    assert sum(ops.count(c) for c in b"=XDd") == len(r), (tag, "reference length")
    # 3. lower-case bytes: a prefix and a suffix only, 'i's before 'd's at either end
    assert re.fullmatch(rb"i*d*[=XID]*i*d*", ops), (tag, "end gaps")
    # 2. '=' on equal bytes, 'X' on different ones; 4. the string re-scores to the score
    i = j = total = 0
    prev = 0
    for op in ops:
        if op in b"=X":
            assert (q[i] == r[j]) == (op == 0x3D), (tag, "column", i, j)
            total += match if op == 0x3D else mismatch
            i += 1
            j += 1
        elif op in b"Ii":
            i += 1
        else:
            j += 1
        if op in b"ID":
            total -= run_step if op == prev else gap_open
        prev = op
    assert total == score, (tag, "re-scored", total, score)


def ops_to_comp(ops):
    return bytes(0x7C if op == 0x3D else 0x20 for op in ops)
