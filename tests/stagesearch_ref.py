"""Plain Python restatement of the expectimax over the multi-stage n-tuple network of
include/g2048_stagesearch.h.

It needs no arithmetic of its own.  The search of tests/ntsearch_ref.py reads its network only
through `net.V(board)`, and tests/ntstage_ref.py's StagedNet has that method: the stage from the
board's own largest exponent, the fall-through over UNSET entries.  So the reference is the
composition

    Search(StagedNet(tuples, bounds, base), p4)

and this file only names it and adds the counts the GPU tests assert about their inputs.

    s = staged_search(tuples, bounds, base, p4=0.5)     an ntsearch_ref.Search
    values, action = s.root(board, depth)               values[a] None for an illegal move
    actions, values = s.root_batch(boards, depth)       the library's output format (INT64_MIN)
    crossing(s, boards, depth) -> (leaves, crossed)     leaves in another stage than their root
    fall_depths(s, boards, depth) -> [n0, n1, ...]      lookups resolved 0, 1, ... stages down

Anchors (asserted by tests/test_stagesearch.py; values in move order up/down/left/right)
--------------------------------------------------------------------------------------
Spec ((0,),): the index is the clamped exponent of one corner and V(b) = 2 * (val[b0] + val[b3] +
val[b12] + val[b15]) at stage(b), each corner being read by two symmetries.

Table X: bounds (2,), stage 0 lut0[i] = 1024 i; at stage 1 an even i holds 4096 i + 3 and an odd
i is UNSET.  So at stage 1: val[0] = 3, val[1] = 1024 (from stage 0), val[2] = 8195, val[3] = 3072
(from stage 0).

Board A = [1, 1, 0, ...] (stage 0; up is illegal).
  depth 1, by hand
    down  after = 2-tiles in cells 12 and 13, still stage 0: 0 + 2 * 1024 = 2048
    left  after = [2, 0, ...]: the 4 in cell 0 reaches the bound, stage 1.  The corner reads
          val[2] = 8195 twice, the six other reads val[0] = 3: (4 << 10) + 2 * 8195 + 6 * 3 = 20504
    right the mirror image, 20504; the tie goes to the smaller move: action 2.
    The single table lut0 alone gives [-, 2048, 8192, 8192] (tests/ntsearch_ref.py's anchor).
  depth 1: [-, 2048, 20504, 20504] at either p(4)
  depth 2: [-, 23136, 24803, 24803] at p(4) = 0.5, [-, 21497, 22126, 22126] at 0.1
  depth 3: [-, 27020, 28091, 28091] at p(4) = 0.5, [-, 24087, 25024, 25024] at 0.1

Board N = [1,2,1,2, 2,1,2,1, 1,2,1,2, 2,1,2,0] (it holds a 2: stage 1, and so is its whole tree),
p(4) = 0.5; only down and right are legal; action 1.
  depth 1: [-, 34834, -, 34834].  By hand, down: column 3 = [2, 1, 2, 0] slides to [0, 2, 1, 2]
    without a merge.  Corners 1, 0, 2, 2: 2 * (1024 + 3 + 8195 + 8195) = 34834.
  depth 2: [-, 51218, -, 51218].  By hand, down: the afterstate's one empty cell is cell 3.
    a 2 there  rows [1,2,1,1] [2,1,2,2] [1,2,1,1] [2,1,2,2]: no vertical move.  left merges
               4 + 8 + 4 + 8 = 24 and leaves corners 1, 0, 2, 0: 24576 + 2 * (1024 + 3 + 8195 + 3)
               = 43026; right gains 24 too, corners 0, 2, 0, 3: 24576 + 2 * (3 + 8195 + 3 + 3072)
               = 47122.                                                           Vmax = 47122
    a 4 there  rows [1,2,1,2] [2,1,2,2] [1,2,1,1] [2,1,2,2].  left gains 8 + 4 + 8 = 20, corners
               1, 2, 2, 0: 20480 + 34834 = 55314; right gains 20, corners 1, 2, 0, 3: 20480 +
               2 * (1024 + 8195 + 3 + 3072) = 45068; up merges the 4s of column 3 (gain 8),
               corners 1, 3, 2, 0: 8192 + 24588 = 32780; down merges them too, corners 1, 0, 2, 2:
               8192 + 34834 = 43026.                                              Vmax = 55314
    Vafter = floor((1 * 47122 + 1 * 55314) / (2 * 1)) = 51218, and the gain of down is 0.
  depth 3: [-, 69650, -, 69650]

Table Y, a bound reached only inside the tree: bounds (25,), lut0[i] = 1000 i, stage 1 all -77.
Board [24,24,23,23, 22,22,0,0, 1,2,1,2, 0,0,1,1] (root in stage 0), p(4) = 0.5.  Left and right
merge the 24s into a 25, whose afterstate lies in stage 1; the index clamps at 15.
  depth 1: [64096, 8096, 60129545624, 60129545624], action 2
           (left by hand: gain 2^25 + 2^24 + 2^23 + 4 = 58720260, << 10 = 60129546240, and
           V = 8 * -77 = -616)
  depth 2: [60129555044, 42949684632, 60129549464, 60129556632], action 3
"""
from __future__ import annotations

import ntsearch_ref as S
import ntstage_ref as R

INT64_MIN = S.INT64_MIN
MAX_DEPTH = S.MAX_DEPTH


def staged_search(tuples, bounds, base=None, p4=0.5) -> S.Search:
    """The reference: ntsearch_ref's search over ntstage_ref's network."""
    return S.Search(R.StagedNet(tuples, bounds, base=base), p4)


def crossing(search: S.Search, boards, depth):
    """(leaves, crossed): the leaves the kernel walks for `boards` (with repetitions) and how
    many of them lie in another stage than their root."""
    net = search.net
    leaves = crossed = 0
    for b in boards:
        root = net.stage(b)
        for leaf in search.leaf_boards(b, depth):
            leaves += 1
            crossed += net.stage(leaf) != root
    return leaves, crossed


def fall_depths(search: S.Search, boards, depth):
    """counts[k] = the table lookups of the search of `boards` that resolve k stages below the
    leaf's own (an entry UNSET at every stage down to 0 counts at the leaf's stage: the last
    read is of stage 0)."""
    net = search.net
    counts = [0] * net.S
    for b in boards:
        for leaf in search.leaf_boards(b, depth):
            s = net.stage(leaf)
            for t, i in net.indices(leaf):
                k = 0
                while k < s and net.raw(s - k, t, i) is None:
                    k += 1
                counts[k] += 1
    return counts
