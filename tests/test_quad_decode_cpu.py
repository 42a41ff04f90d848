"""CPU: the lane arithmetic of the query's quad read in rotated piece order (grp_kernels.inc quad_piece / quad_decode) as a
plain Python model.  A quad of four lanes reads, in round g, the 64-byte line of quad lane g's probe: lane L loads the
16-byte piece (L - g) & 3.  The model moves dwords exactly as the kernel's exchange does and must deliver, for every
(g, lr), the dword that grp_id_loc names (grp_device.h: dword 3 + lr of the bucket's unit, lr < 13)."""
import itertools

GRP_BUCKET_IDS = 13  # ID slots of a bucket line: dwords 3 .. 15
GRP_UNIT_DW = 32     # dwords of a bucket's 128-byte unit (the quad reads its first line)


def grp_id_loc(b, lr):
    return b * GRP_UNIT_DW + 3 + lr if lr < GRP_BUCKET_IDS else b * GRP_UNIT_DW


def quad_piece(sub, g):
    return (sub - g) & 3


def quad_exchange(lines, lrs):
    """lines[g]: the 16 dwords of lane g's line, lrs[g]: lane g's local rank -> per lane (header piece, ID word)"""
    # the loads: pc[L][g] = the piece lane L holds of round g
    pc = [[lines[g][4 * quad_piece(L, g): 4 * quad_piece(L, g) + 4] for g in range(4)] for L in range(4)]
    slot = [3 + min(lr, GRP_BUCKET_IDS - 1) for lr in lrs]
    src = [(L + (slot[L] >> 2)) & 3 for L in range(4)]  # computed once per lane, used in every round
    out = []
    for L in range(4):
        per_round = []
        for g in range(4):
            comp = slot[g] & 3                                 # lane g's slot, broadcast
            word = [pc[lane][g][comp] for lane in range(4)]    # every lane picks that component of its round-g piece
            per_round.append(word[src[L]])                     # ds_bpermute: lane L pulls from ITS source lane
        out.append((pc[L][L], per_round[L]))                   # lane L keeps round L
    return out


def test_each_round_reads_one_whole_line():
    for g in range(4):
        assert sorted(quad_piece(L, g) for L in range(4)) == [0, 1, 2, 3]
        assert quad_piece(g, g) == 0  # the header piece arrives in the lane that owns the probe


def test_source_lane_and_component_against_grp_id_loc():
    for g, lr in itertools.product(range(4), range(GRP_BUCKET_IDS + 4)):
        b = 1000 + 7 * g
        # every dword of every line is its own global dword index; the other lanes probe other buckets at other ranks
        buckets = [b if L == g else 50 + L for L in range(4)]
        lrs = [lr if L == g else (lr + 3 * L + 1) % GRP_BUCKET_IDS for L in range(4)]
        lines = [[bk * GRP_UNIT_DW + d for d in range(16)] for bk in buckets]
        got = quad_exchange(lines, lrs)
        for L in range(4):
            header, word = got[L]
            assert header == lines[L][:4], (g, lr, L)
            want = grp_id_loc(buckets[L], min(lrs[L], GRP_BUCKET_IDS - 1))  # (lr >= 13: the slot is clamped, the ID comes from the overflow table)
            assert word == want, (g, lr, L)
            if lrs[L] >= GRP_BUCKET_IDS:
                assert grp_id_loc(buckets[L], lrs[L]) == buckets[L] * GRP_UNIT_DW


def test_slot_three_is_the_lanes_own_header_piece():
    for L in range(4):
        assert (L + ((3 + 0) >> 2)) & 3 == L and (3 + 0) & 3 == 3  # ids[0]: component w of piece 0, no other lane involved
