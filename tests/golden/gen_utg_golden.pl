#!/usr/bin/env perl
# Golden-vector generator for the unitig consensus (bam2cns --utg-mode).
#
# Runs the REFERENCE consensus engine (Sam::Seq / Sam::Alignment / Fastq::Seq / Fasta::Seq from
# the read-only reference checkout, $PROOVREAD_REFERENCE/lib) the way bin/bam2cns does in unitig
# mode: the class settings of bam2cns:227-237, one Sam::Seq per reference read with add_aln for
# every alignment (bam2cns:339-355), then generate_consensus (bam2cns:375-455) statement by
# statement.  Cases come from a case file (tests/utg_cases.py describes the format); the output
# holds each case's FASTQ record, trace, surviving alignment names and overlap windows.
#
# Determinism: Sam::Seq::alns is overridden to return alignments in ascending internal id
# (arrival) order, the canonical order the library uses.  filter_contained_alns sorts Perl's
# hash order by length only, so every two alignments of a case have different lengths; the
# fixture is committed only when three PERL_HASH_SEED values give the same bytes (regen_utg.sh).
#
# Usage: perl gen_utg_golden.pl utg_cases.txt > utg_expected.txt
use strict;
use warnings;

BEGIN {
    my $ref = $ENV{PROOVREAD_REFERENCE} or die "set PROOVREAD_REFERENCE to the reference checkout\n";
    unshift @INC, "$ref/lib";
}
use Sam::Seq;
use Sam::Alignment;
use Fastq::Seq;
use Fasta::Seq;

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
    my ($name, $flags, $cfg, $ref_lines, $sam_lines) = @_;
    my %o = (use_ref_qual => 1, qual_weighted => 0, max_ins_length => 0);
    my @f = split ' ', $flags;
    while (@f) {
        my $k = shift @f;
        if    ($k eq '--qual-weighted')   { $o{qual_weighted} = 1 }
        elsif ($k eq '--no-use-ref-qual') { $o{use_ref_qual} = 0 }
        elsif ($k eq '--invert-scores')   { $o{invert_scores} = 1 }
        elsif ($k eq '--ignore-hcr')      { $o{ignore_mcr} = 1 }
        elsif ($k eq '--utg-mode')        { }
        elsif ($k eq '--rep-coverage')    { $o{rep_coverage} = shift @f }
        elsif ($k eq '--min-ncscore')     { $o{min_ncscore} = shift @f }
        elsif ($k eq '--fallback-phred')  { $o{fallback_phred} = shift @f }
        elsif ($k eq '--max-ins-length')  { $o{max_ins_length} = shift @f }
        elsif ($k eq '--coverage')        { shift @f }
        else { die "unknown flag $k\n" }
    }
    my %cfg = ('sr-trim' => 1, 'sr-indel-taboo-length' => 7, 'sr-indel-taboo' => 0.1, map { split /=/ } split ' ', $cfg);
    # bam2cns:227-237
    Sam::Seq->Trim($cfg{'sr-trim'});
    Sam::Seq->InDelTabooLength($cfg{'sr-indel-taboo-length'});
    Sam::Seq->InDelTaboo($cfg{'sr-indel-taboo'});
    Sam::Seq->MaxCoverage(1);
    Sam::Seq->BinSize(20);
    Sam::Seq->PhredOffset(33);
    Sam::Seq->MaxInsLength($o{max_ins_length});
    Sam::Seq->FallbackPhred(defined $o{fallback_phred} ? $o{fallback_phred} : 1);
    Sam::Seq->RepCoverage(defined $o{rep_coverage} ? $o{rep_coverage} : 0);
    Sam::Seq->MinNCScore($o{min_ncscore});
    $Sam::Alignment::InvertScores = $o{invert_scores} ? 1 : 0;

    my $out = ">>CASE $name\n";
    my $ok  = eval {
        my ($ref, $fastq);
        if ($ref_lines->[0] =~ /^@/) {
            $ref = Fastq::Seq->new(@$ref_lines, phred_offset => 33);
            $fastq = 1;
        } else {
            my ($id, $desc) = $ref_lines->[0] =~ /^>(\S+)\s?(.*)$/;
            $ref = Fasta::Seq->new(id => $id, desc => $desc, seq => $ref_lines->[1], seq_head => $ref_lines->[0]);
        }
        my $use_ref_qual = $fastq ? $o{use_ref_qual} : 0;        # bam2cns:258
        my $ignore_mcr   = $fastq ? $o{ignore_mcr}   : 1;        # bam2cns:259-262
        my $sso = Sam::Seq->new(id => $ref->id, len => length($ref->seq), ref => $ref);
        $sso->add_aln(Sam::Alignment->new($_)) for @$sam_lines;   # bam2cns:349-351

        # bam2cns:378-391
        my @mcrs;
        if (!$ignore_mcr) {
            if (my $mcrs = $ref->desc) {
                while ($mcrs =~ /MCR\d+:(\d+),(\d+)/g) { push @mcrs, [$1, $2]; }
            }
        }
        # bam2cns:394-395
        $sso->filter_by_ncscore if defined $o{min_ncscore};
        $sso->filter_rep_region_alns if defined $o{rep_coverage};
        # bam2cns:398-422
        my @owin;
        $sso->filter_contained_alns;
        # the runs of columns whose coverage is not below --rep-coverage (undef compares as 0)
        my @cov  = $sso->coverage(1);
        my $cmax = $o{rep_coverage};
        my $start;
        for my $i (0 .. $#cov, scalar @cov) {
            my $hi = $i < @cov && !($cov[$i] < $cmax);
            if ($hi && !defined $start) { $start = $i; }
            elsif (!$hi && defined $start) { push @owin, [$start, $i - $start]; undef $start; }
        }
        # bam2cns:434-438
        my $con = $sso->consensus(
            use_ref_qual  => $use_ref_qual,
            ignore_coords => [@mcrs, @owin],
            qual_weighted => $o{qual_weighted},
        );
        my $rec = "$con";
        chomp $rec;
        my @kept = map { $_->qname } $sso->alns;
        $out .= ">>FASTQ\n$rec\n>>TRACE\n" . ($con->{trace} // '') . "\n>>KEPT\n@kept\n>>WIN\n"
            . join(' ', map { "$_->[0],$_->[1]" } @owin) . "\n";
        1;
    };
    if (!$ok) {
        print STDERR "$name: $@" if $ENV{GOLDEN_DEBUG};
        $out = ">>CASE $name\n>>ERROR 1\n";
    }
    print $out . ">>END\n";
}

my ($name, $flags, $cfg, @ref, @sam);
my $sect = '';
while (my $line = <>) {
    chomp $line;
    next if $line =~ /^#/ && !$sect;   # the header comment
    if ($line =~ /^>>CASE (.*)/) { $name = $1; $flags = ''; $cfg = ''; @ref = (); @sam = (); $sect = ''; }
    elsif ($line =~ /^>>PARAM flags ?(.*)/) { $flags = $1; }
    elsif ($line =~ /^>>PARAM cfg ?(.*)/) { $cfg = $1; }
    elsif ($line eq '>>REF') { $sect = 'ref'; }
    elsif ($line eq '>>SAM') { $sect = 'sam'; }
    elsif ($line eq '>>END') { run_case($name, $flags, $cfg, [@ref], [@sam]); $sect = ''; }
    elsif ($sect eq 'ref') { push @ref, $line; }
    elsif ($sect eq 'sam') { push @sam, $line if length $line; }
}
