"""The scoring parameters the aligner is tested at besides 2 / -2 / 1, shared by tests/test_align_params_host.py (the host
aligner against the oracle's and a plain score loop) and tests/test_gpu_align_params.py (every GPU entry form and route against
the host aligner).  gap_open is per pair (ioc_host_gap_open: 2 .. 5), so one parameter set meets four (cm, cx, gd) classes:
cm = match + gap_extend + gap_open and cx = mismatch + gap_extend + gap_open are what the forward kernels add on a diagonal step,
gd = gap_open - gap_extend what they subtract where a gap may open."""
from isonclust2_amd import _lib

GAP_OPENS = (2, 3, 4, 5)
DEFAULT = (2, -2, 1)

# (match, mismatch, gap_extend): why it is here
PARAM_TABLE = {
    (2, -2, 1): "the default: every score even, whole classes of ties cannot occur",
    (1, -1, 1): "tie-rich: diagonal, E and F meet at equal scores",
    (5, -4, 2): "tie-rich, and gap_open == gap_extend at gap_open 2: one gap of a + b costs what gaps of a and of b do",
    (2, -2, 0): "extending is free: gd = gap_open, long gaps, no slant",
    (2, -6, 1): "cx = gap_open - 5 crosses 0 between the gap-open classes: 5 profile, 2 .. 4 comparing kernel",
    (250, -2, 1): "cm = 251 + gap_open crosses 255: 5 comparing kernel, 2 .. 4 profile but far above version 2's 16-bit rise",
    (2, -2, 3): "gap_extend above gap_open 2 (gd = -1), equal to gap_open 3 (gd = 0)",
    (2, -2, 6): "gap_extend above every gap_open: gd = -4 .. -1",
    (0, -1, 1): "no reward for a match: the best score is 0, ties everywhere",
    (3, -1, 2): "tie-rich: odd and even scores mix, gap_open == gap_extend at 2",
    (1, -3, 5): "gap_extend above open, cx = 4 .. 7, gd = -3 .. 0",
}
PARAM_SETS = list(PARAM_TABLE)
PARAM_IDS = ["%d_%d_%d" % p for p in PARAM_SETS]

ROUTE_COMPARE, ROUTE_PROFILE, ROUTE_V2 = 0, 1, 2


def route(params, gap_open):
    """ioc_host_align_route: the kernel family of a pair of four-letter sequences (0 comparing, 1 profile with 32-bit cells, 2
    version 2 may take it)."""
    return _lib.load().ioc_host_align_route(params[0], params[1], params[2], gap_open)


def routes(params):
    """{gap_open: route} of one parameter set."""
    return {go: route(params, go) for go in GAP_OPENS}
