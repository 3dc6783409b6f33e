"""The read alphabet as the reference's text states it, in plain Python: what each of the 256 byte values does in a read.

A reading of the reference, not an execution of it, and it shares no code with the product's tables (ga_host.cpp), the oracle or
cell_dp_checker.py.  Three rules:

* forwards -- characterMatch (GraphAligner.h:2039-2110): the 15 IUPAC letters A C G T N R Y K M S W B D H V in either case match the
  graph bases of their sets; every other byte, 'U' and 'u' included, takes the default branch, assert(false).  The forward part's
  match vectors are built with it for every row (:2338-2351), so such a byte anywhere in a forward part ends the read in the
  assertion.
* backwards -- ReverseComplement (CommonUtils.cpp:60-136) turns the read's prefix into the backward part: the complement, UPPER
  case, of A C T G N U R Y K M S W B V D in either case ('U' -> 'A').  'H' / 'h' append 'D' and then fall through, without a break,
  into the default branch's assert(false) (:128-132); every byte outside the list asserts as well.  The call is eager over the whole
  prefix (GraphAligner.h:2992).
* along the trace -- getTraceInfo (:463, :690-780) walks the finished trace with the ORIGINAL read and calls characterMatch on
  sequence[newpos.second] for every diagonal step.  A byte that ReverseComplement accepted but characterMatch does not ('U', 'u')
  therefore still asserts when the backward trace crosses its row diagonally.

  Why read position 0 escapes: getTraceInfoInner's loop starts at i = 1 (:721) and looks at trace[i] only as `newpos`; trace[0] is
  never given to characterMatch.  The backward trace is reversed into read coordinates (reverseTrace, :3026-3037, :3090), so its
  element 0 is the cell of the backward part's LAST row, read position 0; any further cell on read row 0 is reached with
  newpos.second == oldpos.second, a DELETION, which is typed before characterMatch is asked (:758-761).  The forward trace's
  element 0 (the seed's own base) is skipped the same way, but the forward part has asserted on it long before.  So the exact
  condition is: the byte lies in the backward part, is outside characterMatch, and its read position is > 0.

  (For positions > 0 the model takes the step onto the row to be diagonal.  With one substituted byte in an otherwise error-free
  read that is the only path of the minimal score: leaving the diagonal costs an insertion and a deletion.  The tests check it
  against the oracle on every such probe.)

The exact comparison.  Next to characterMatch the reference compares raw characters once: `previousEq`, graph base ==
sequence[j-1] (:1503, :1540, used in :1369), on the part as getSplitAlignment built it.  A forward part holds the read's own bytes,
so only upper-case A C G T can be equal to a graph base there; a backward part holds ReverseComplement's output, upper case, so
'a' is equal to a graph 'T' backwards although it is equal to nothing forwards; padding rows hold 'N', equal to nothing.
exact_letter gives the graph base a row's character is raw-equal to, or None.  (No alignment result has been seen to depend on it:
DESIGN.md section 5.  The tables that carry it are pinned byte by byte all the same.)

Which part holds a read position (getSplitAlignment, :2989-3021), for a seed at read position s of a read of n bases on a graph
without node overlap: the backward part is the reverse complement of positions 0 .. s-1 and exists when s > 0; the forward part is
positions s .. n-1 and exists when s < n - 1.  A seed on the last base leaves that base in NO part: no rule ever looks at it.
A part shorter than 193 rows asserts on its own (samplingFrequency, :2965 and :906); the model refuses such reads.
"""

GA_S_OK = 0
GA_S_ASSERTION = 1

# characterMatch, GraphAligner.h:2044-2103, case by case
_MATCH = {
    "A": "A", "T": "T", "C": "C", "G": "G", "N": "ACGT",
    "R": "AG", "Y": "CT", "K": "GT", "M": "CA", "S": "CG", "W": "AT",
    "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG",
}
# ReverseComplement, CommonUtils.cpp:68-126, case by case ('H' is listed there but runs on into assert(false))
_COMPLEMENT = {
    "A": "T", "C": "G", "T": "A", "G": "C", "N": "N", "U": "A",
    "R": "Y", "Y": "R", "K": "M", "M": "K", "S": "S", "W": "W",
    "B": "V", "V": "B", "D": "H",
}
_BASE_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def forward_set(byte):
    """the graph bases byte value `byte` matches in a forward part; None: characterMatch asserts"""
    c = chr(byte)
    for letter, bases in _MATCH.items():
        if c == letter or c == letter.lower():
            return frozenset(bases)
    return None


def backward_char(byte):
    """what byte value `byte` becomes in a backward part (one upper-case letter); None: ReverseComplement asserts"""
    c = chr(byte)
    for letter, comp in _COMPLEMENT.items():
        if c == letter or c == letter.lower():
            return comp
    return None


def exact_letter(byte, part):
    """the one graph base that the character of a row holding `byte` is raw-equal to (`previousEq`), or None; part: "forward" |
    "backward"; a byte the part's rule refuses has no row"""
    c = chr(byte) if part == "forward" else backward_char(byte)
    return c if c in _BASE_COMPLEMENT else None


def trace_accepts(byte):
    """getTraceInfo's characterMatch on the original read byte"""
    return forward_set(byte) is not None


def part_of(n, seed_pos, pos):
    """-> ("backward" | "forward" | None, row of the part) for read position `pos` of a read of n bases seeded at seed_pos"""
    assert 0 <= seed_pos < n and 0 <= pos < n
    if seed_pos > 0 and pos < seed_pos:
        return "backward", seed_pos - 1 - pos
    if seed_pos < n - 1 and pos >= seed_pos:
        return "forward", pos - seed_pos
    return None, None


def part_lengths(n, seed_pos):
    """(rows of the backward part, rows of the forward part); 0 = the part does not exist"""
    return (seed_pos if seed_pos > 0 else 0), (n - seed_pos if seed_pos < n - 1 else 0)


def expected(path, seed_pos, pos, byte):
    """path: the graph bases (bytes, upper case ACGT) that an error-free read was copied from, base for base, on a linear graph;
    the read is `path` with position `pos` replaced by `byte`, seeded at seed_pos on the node that holds path[seed_pos].
    -> (ABI status, total score; None with an assertion)"""
    n = len(path)
    for rows in part_lengths(n, seed_pos):
        if rows and rows < 193:
            raise ValueError("a part of %d rows asserts by itself: outside this model" % rows)
    part, _ = part_of(n, seed_pos, pos)
    base = chr(path[pos])
    assert base in _BASE_COMPLEMENT
    if part is None:
        return GA_S_OK, 0
    if part == "forward":
        bases = forward_set(byte)
        if bases is None:
            return GA_S_ASSERTION, None
        return GA_S_OK, 0 if base in bases else 1
    turned = backward_char(byte)
    if turned is None:
        return GA_S_ASSERTION, None
    if not trace_accepts(byte) and pos > 0:
        return GA_S_ASSERTION, None
    # the backward part meets the other strand: the turned letter against the complement of the graph base
    return GA_S_OK, 0 if _BASE_COMPLEMENT[base] in _MATCH[turned] else 1
