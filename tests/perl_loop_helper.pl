#!/usr/bin/env perl
# Test helper for tests/test_perl_loop.py: the host logic of the Perl correction loop
# (perl/lib/Prgpu/{Tasks,Control,ShortReads,Loop}.pm) on inputs given as JSON, results as JSON,
# for comparison with the Python modules they were ported from.  No GPU.
#
#   perl_loop_helper.pl tables IN.json    {tasks, modes, lengths} -> per task both option structs
#       (every field, through Prgpu::seed_opts / Prgpu::sw_opts), sr_coverage, hcr_mask,
#       detect_chimera; bin_size per mode; mode_for per length; the mode task lists
#   perl_loop_helper.pl control IN.json   {grid: [[c, tc], ...], sampling, shortcut: [{tasks, tc,
#       frac, fracs, shortcut_frac, min_gain}]} -> cov2seqchunker of one Sampler over the grid,
#       mask_shortcut's result, task list and fraction list per case
#   perl_loop_helper.pl sample IN.json    {file, chunk_number, scs: [sc or null, ...]} -> {n,
#       min_length, samples: [{ranges, off}]}
#   perl_loop_helper.pl read_long IN.json {records, stubby} -> {ids, seqs, quals, ignored} or {error}
#   perl_loop_helper.pl outputs IN.json   {ids, seqs, quals, chim, ignored, pre} -> writes the files
use strict;
use warnings;
use FindBin;
use lib "$FindBin::RealBin/../perl/lib";
use JSON::PP;
use Prgpu;
use Prgpu::Tasks;
use Prgpu::Control;
use Prgpu::ShortReads;
use Prgpu::Loop;

my ($mode, $file) = @ARGV;
open my $fh, '<', $file or die "$file: $!\n";
my $in = decode_json(do { local $/; <$fh> });
close $fh;
my $json = JSON::PP->new->canonical->allow_nonref;
my $out;

if ($mode eq 'tables') {
    my %t;
    for my $task (@{$in->{tasks}}) {
        my ($so, $wo) = Prgpu::Tasks::options($task);
        $t{$task} = {seed => Prgpu::seed_opts($so), sw => Prgpu::sw_opts($wo),
                     sr_coverage => Prgpu::Tasks::sr_coverage($task), hcr_mask => Prgpu::Tasks::hcr_mask($task),
                     detect_chimera => Prgpu::Tasks::detect_chimera($task)};
    }
    $out = {tasks => \%t, bin_size => {map { $_ => Prgpu::Tasks::bin_size($_) } @{$in->{modes}}},
            mode_for => {map { $_ => Prgpu::Tasks::mode_for($_) } @{$in->{lengths}}},
            mode_tasks => {map { $_ => $Prgpu::Tasks::MODE_TASKS{$_} } @{$in->{modes}}}};
} elsif ($mode eq 'control') {
    my $s = Prgpu::Control::Sampler->new(sampling => $in->{sampling});
    my @sc = map { $s->cov2seqchunker(@$_) } @{$in->{grid}};
    my @cases;
    for my $c (@{$in->{shortcut}}) {
        my @tasks = @{$c->{tasks}};
        my @fracs = @{$c->{fracs}};
        my $res = Prgpu::Control::mask_shortcut(\@tasks, $c->{tc}, $c->{frac}, \@fracs, $c->{shortcut_frac}, $c->{min_gain});
        push @cases, {res => $res, tasks => \@tasks, fracs => \@fracs};
    }
    $out = {sc => \@sc, shortcut => \@cases};
} elsif ($mode eq 'sample') {
    my $srs = Prgpu::ShortReads->new(Prgpu::Loop::slurp($in->{file}), $in->{chunk_number});
    my @samples;
    for my $sc (@{$in->{scs}}) {
        my ($rg, $off) = $srs->sample_ranges($sc);
        push @samples, {ranges => $rg, off => $off};
    }
    $out = {n => $srs->n, min_length => $srs->min_length, pool => unpack('H*', $srs->{pool}), samples => \@samples};
} elsif ($mode eq 'read_long') {
    my @r = eval { Prgpu::Loop::read_long($in->{records}, $in->{stubby}) };
    $out = $@ ? {error => $@} : {ids => $r[0], seqs => $r[1], quals => $r[2], ignored => $r[3]};
} elsif ($mode eq 'outputs') {
    Prgpu::Loop::write_outputs($in, $in->{pre});
    $out = {};
} else {
    die "usage: perl_loop_helper.pl tables|control|sample|read_long|outputs IN.json\n";
}
print $json->encode($out), "\n";
