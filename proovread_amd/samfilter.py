"""`samfilter`-compatible line filter: SAM on stdin to SAM on stdout, for the stream of a mapper
that prints no SEQ / QUAL on secondary lines (`bwa mem -a`), before it is sorted.

    bwa mem -a ref.fa reads.fq | python -m proovread_amd.samfilter | samtools sort ...

In stream order, as the reference tool:

* header lines pass through;
* unmapped records (FLAG 0x4) are dropped;
* the last record that is not secondary (FLAG 0x100 clear) is the donor;
* a secondary record with SEQ `*` takes the donor's SEQ and QUAL, reverse-complemented
  (A<->T, C<->G in either case, other letters kept) and reversed when their strands differ; it
  is an error unless a donor of the same QNAME precedes it;
* a `*` QUAL becomes `?` x the length of SEQ (the donor keeps that QUAL for what follows).

This is host code.  A coordinate-sorted file has lost the stream order this filter relies on:
`correct --bam FILE --restore-secondary-seq` finds the donors by name on the device instead
(DESIGN.md §10).
"""
from __future__ import annotations

import sys
from typing import Iterable, Iterator, List, Optional

UNMAPPED, REVERSE, SECONDARY = 0x4, 0x10, 0x100
QUAL_DEFAULT = "?"
_COMPLEMENT = str.maketrans("ATGCatgc", "TACGtacg")


class SamfilterError(RuntimeError):
    pass


def reverse_complement(seq: str) -> str:
    return seq.translate(_COMPLEMENT)[::-1]


def filter_lines(lines: Iterable[str]) -> Iterator[str]:
    """The filtered stream; lines come and go with their newline."""
    donor: Optional[List[str]] = None
    in_header = True
    for line in lines:
        if in_header and line.startswith("@"):
            yield line
            continue
        in_header = False
        f = line.rstrip("\n").split("\t")
        flag = int(f[1])
        if flag & UNMAPPED:
            continue
        if not flag & SECONDARY:
            donor = f
        elif f[9] == "*":
            if donor is None:
                raise SamfilterError("SAM started with secondary alignment without seq/qual and without preceding "
                                     "primary alignment")
            if donor[0] != f[0]:
                raise SamfilterError("Secondary alignment without seq/qual and without primary alignment\n" + line)
            if (flag ^ int(donor[1])) & REVERSE:
                f[9], f[10] = reverse_complement(donor[9]), donor[10][::-1]
            else:
                f[9], f[10] = donor[9], donor[10]
        if f[10] == "*":
            f[10] = QUAL_DEFAULT * len(f[9])
        yield "\t".join(f) + "\n"


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if argv:
        sys.stderr.write("usage: samfilter < in.sam > out.sam\n")
        return 2
    try:
        for out in filter_lines(sys.stdin):
            sys.stdout.write(out)
    except SamfilterError as e:
        sys.stderr.write(f"[samfilter] {e}\n")
        return 255
    return 0


if __name__ == "__main__":
    sys.exit(main())
