#!/usr/bin/env perl
# Golden-vector generator for siamaera's record editing (bin/siamaera:365-393, :407-433).
#
# Loads the REFERENCE modules Fastq::Seq and Fasta::Seq from the read-only checkout (default
# /root/reference/lib), applies to each case what siamaera applies to a trimmed read,
#     tail form:  $fa = $fa->substr_seq($j);     $fa->desc_append("SIAMAERA:$j,$sl");
#     head form:  $fa = $fa->substr_seq(0, $j);  $fa->desc_append("SIAMAERA:0,$j");
# and prints the record the way siamaera does (print "$fa").
#
# Output: per case a line "CASE <kind> <form> <j> <head> <seq> <qual>" (tab separated, qual
# "-" for FASTA), the printed record, and a line "END".
#
# Usage: perl gen_siamaera_golden.pl > siamaera_records.txt
# Only this container runs it; its output is committed as the fixture.
use strict;
use warnings;

BEGIN {
    my $ref = $ENV{PROOVREAD_REFERENCE} || '/root/reference';
    unshift @INC, "$ref/lib";
}
use Fastq::Seq;
use Fasta::Seq;

$SIG{__WARN__} = sub { };

my $seq  = 'ACGTTGCAAGGCTTACCGATAGGCATTACGGATCCAGTTAGCAAT';
my $qual = join('', map { chr(33 + ($_ * 7) % 41) } 1 .. length($seq));

my @cases = (
    ['fastq', 'tail', 17, '@read/1 some description', $seq, $qual],
    ['fastq', 'head', 23, '@read/1 some description', $seq, $qual],
    ['fastq', 'tail', 9,  '@read_2',                  $seq, $qual],
    ['fastq', 'head', 30, '@read_2',                  $seq, $qual],
    ['fastq', 'tail', 12, '@r3 SUBSTR:5,40',          $seq, $qual],
    ['fasta', 'tail', 17, '>contig_7 len=45 x',       $seq, ''],
    ['fasta', 'head', 23, '>contig_7 len=45 x',       $seq, ''],
    ['fasta', 'tail', 9,  '>c8',                      $seq, ''],
    ['fasta', 'head', 30, '>c8',                      $seq, ''],
);

for my $c (@cases) {
    my ($kind, $form, $j, $head, $s, $q) = @$c;
    my $fa = $kind eq 'fastq'
        ? Fastq::Seq->new("$head\n$s\n+\n$q\n", phred_offset => 33)
        : Fasta::Seq->new(seq_head => $head, seq => $s);
    my $sl = length($fa->seq);
    if ($form eq 'tail') {
        $fa = $fa->substr_seq($j);
        $fa->desc_append("SIAMAERA:$j,$sl");
    } else {
        $fa = $fa->substr_seq(0, $j);
        $fa->desc_append("SIAMAERA:0,$j");
    }
    print join("\t", 'CASE', $kind, $form, $j, $head, $s, length($q) ? $q : '-'), "\n";
    print "$fa";
    print "END\n";
}
