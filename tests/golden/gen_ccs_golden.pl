#!/usr/bin/env perl
# Golden-vector generator for the ccs-1 consensus.
#
# Runs the REFERENCE consensus engine (Sam::Seq / Sam::Alignment / Fastq::Seq from the
# read-only reference checkout, $PROOVREAD_REFERENCE/lib) the way bin/ccseq does
# (ccseq:214-217 class settings, :244-249 one Sam::Seq per reference subread, :438 add_aln,
# :267-271 consensus and desc_append) on every case of a case file (tests/golden/casefmt.py)
# and prints the expected records.  Alignments are fed from the case's SAM text in arrival order.
#
# Determinism (SURVEY.md §8c): Sam::Seq::alns is overridden to return alignments in ascending
# internal id (arrival) order, the canonical order the C oracle and the library use.
#
# Usage: perl gen_ccs_golden.pl ccs_cases.txt > ccs_expected.txt
use strict;
use warnings;

BEGIN {
    my $ref = $ENV{PROOVREAD_REFERENCE} or die "set PROOVREAD_REFERENCE to the reference checkout\n";
    unshift @INC, "$ref/lib";
}
use Sam::Seq;
use Sam::Alignment;
use Fastq::Seq;

{
    no warnings 'redefine';
    *Sam::Seq::alns = sub {
        my ($self, $by_pos) = @_;
        return scalar keys %{ $self->{_alns} } unless wantarray;
        my @a = map { $self->{_alns}{$_} } sort { $a <=> $b } keys %{ $self->{_alns} };
        @a = sort { $a->{pos} <=> $b->{pos} } @a if $by_pos;
        return @a;
    };
}

$SIG{__WARN__} = sub { };   # the reference warns on undef lookups it tolerates

sub run_case {
    my ($name, $ref_lines, $sam_lines) = @_;
    Sam::Seq->Trim(1);               # ccseq:214
    Sam::Seq->InDelTaboo(0.001);     # ccseq:215
    Sam::Seq->PhredOffset(33);       # ccseq:217

    my $fq  = Fastq::Seq->new(@$ref_lines, phred_offset => 33);
    my $out = ">>CASE $name\n";
    my $ok  = eval {
        my $sso = Sam::Seq->new(id => $fq->id, len => length($fq->seq), ref => $fq, CCS => 'primary');
        $sso->add_aln(Sam::Alignment->new($_)) for @$sam_lines;
        my $con = $sso->consensus(use_ref_qual => 1, qual_weighted => 1);
        $con->desc_append("CCS:" . $sso->{CCS});
        my $rec = "$con";
        chomp $rec;
        $out .= ">>FASTQ\n$rec\n>>TRACE\n" . ($con->{trace} // '') . "\n>>CHIM\n";
        1;
    };
    if (!$ok) {
        print STDERR "$name: $@" if $ENV{GOLDEN_DEBUG};
        $out = ">>CASE $name\n>>ERROR 1\n";
    }
    print $out . ">>KEPT\n\n>>END\n";
}

my ($name, @ref, @sam, $sect);
while (my $line = <>) {
    chomp $line;
    if ($line =~ /^>>CASE (.*)/) { $name = $1; @ref = (); @sam = (); $sect = ''; }
    elsif ($line =~ /^>>PARAM /) { }
    elsif ($line eq '>>REF') { $sect = 'ref'; }
    elsif ($line eq '>>SAM') { $sect = 'sam'; }
    elsif ($line eq '>>END') { run_case($name, [@ref], [@sam]); }
    elsif ($sect eq 'ref') { push @ref, $line; }
    elsif ($sect eq 'sam') { push @sam, $line if length $line; }
}
