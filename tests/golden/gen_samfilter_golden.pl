#!/usr/bin/env perl
# Golden-vector generator for the samfilter drop-in (proovread_amd/samfilter.py).
#
# The reference's bin/samfilter needs Log::Log4perl, which is not everywhere; the modules it
# does its work with load without it.  This script drives them record by record -- Sam::Parser
# for the lines, Sam::Alignment for the fields and the printed form, Fasta::Seq's
# Reverse_complement for the other strand -- over every case of a case file and prints what the
# tool's stream would hold, or `!die` where the tool gives up.
#
# Case file: `#case NAME` starts a case, the lines up to the next one are its SAM stream.
# Usage: PROOVREAD_REFERENCE=<checkout> perl gen_samfilter_golden.pl samfilter_cases.txt > samfilter_expected.txt
use strict;
use warnings;

BEGIN {
    die "PROOVREAD_REFERENCE (the reference checkout) is not set\n" unless $ENV{PROOVREAD_REFERENCE};
    unshift @INC, "$ENV{PROOVREAD_REFERENCE}/lib";
}
use Sam::Parser;
use Sam::Alignment ':flags';
use Fasta::Seq;

sub filter_case {
    my ($text) = @_;
    open(my $fh, '<', \$text) or die $!;
    my $sp = Sam::Parser->new(fh => $fh);
    my @out;
    while (defined(my $h = $sp->next_header_line)) { push @out, $h }
    my $donor;
    while (my $aln = $sp->next_aln) {
        next if $aln->{flag} & UNMAPPED;
        if ($aln->{flag} & SECONDARY_ALIGNMENT) {
            if ($aln->seq eq '*') {
                return undef unless defined $donor && $donor->qname eq $aln->qname;
                my $other = ($aln->{flag} & REVERSE_COMPLEMENT) != ($donor->{flag} & REVERSE_COMPLEMENT);
                $aln->seq($other ? Fasta::Seq->Reverse_complement($donor->seq) : $donor->seq);
                $aln->qual($other ? scalar reverse($donor->qual) : $donor->qual);
            }
        } else {
            $donor = $aln;
        }
        $aln->qual('?' x length($aln->seq)) if $aln->qual eq '*';
        push @out, "$aln";
    }
    return join('', @out);
}

my ($name, $text, @cases);
while (my $l = <>) {
    if ($l =~ /^#case\s+(\S+)/) {
        push @cases, [$name, $text] if defined $name;
        ($name, $text) = ($1, '');
    } elsif (defined $name) {
        $text .= $l;
    }
}
push @cases, [$name, $text] if defined $name;
for my $c (@cases) {
    my $out = filter_case($c->[1]);
    print "#case $c->[0]\n", defined $out ? $out : "!die\n";
}
