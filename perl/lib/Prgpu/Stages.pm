package Prgpu::Stages;

# The device stages of the correction loop for a Perl host, at world 1: what GpuStages
# (proovread_amd/correct.py) is to the Python driver, over the same resident entry points.
# The loop's state -- the current long reads, their qualities and the mapping reference, and
# the whole short-read input -- stays in HBM between tasks; a task sends its record ranges and
# the sample's offsets and brings back two counters, or the finish task's chimera rows.
#
#   my $st = Prgpu::Stages->new(Prgpu::Context->new(0));
#   $st->load(\@ids, \@seqs, \@quals);               # read-long's output (pr_lrset_load)
#   $st->load_short_reads($nt4_pool, \@off);         # the short-read input, once (pr_srset_load)
#   my $r = $st->task('bwa-sr-1', \@ranges, \@sr_off, \%cns_params, [$bin, $len],
#                     [$hcr_mask, $min_sr]);         # -> {n_tasks, chim => [], bpt, bpn}
#   my $f = $st->task('bwa-sr-finish', \@ranges, \@sr_off, \%cns_params, [$bin, $len], undef);
#   my ($ids, $seqs, $quals) = $st->reads;
#
# The calls of one task, in GpuStages.task's order:
#   index     lrset_index: the seed index of the mapping reference (finish: of the reads)
#   seeding   seed_map_sampled: the sample gathered and seeded on the device, seeds kept in HBM
#   launch    iter_upload_lrset + iter_launch: SW, -b/-l filter, hand-off, consensus
#   finish    iter_chim: the chimera rows, formatted here as Prgpu::chim_lines formats them
#   regular   iter_mask into a device int64[2], read back: bpt, bpN
#   commit    lrset_commit: the consensus (regular: and its masked copy) replaces the set's reads

use strict;
use warnings;
use Time::HiRes ();
use Prgpu;
use Prgpu::Tasks;

use constant { MAP => 0, READS => 1, COMMIT_MASK => 1 };

sub new {
    my ($class, $ctx) = @_;
    die "Prgpu::Stages: a Prgpu::Context is required\n" unless ref $ctx && $ctx->can('handle');
    return bless {ctx => $ctx, h => $ctx->handle, ids => [], stats => 0, device_ms => 0}, $class;
}

sub DESTROY {
    my $self = shift;
    Prgpu::dev_free($self->{h}, $self->{stats}) if $self->{stats} && $self->{ctx}{h};
    $self->{stats} = 0;
}

sub _off {
    my @off = (0);
    push @off, $off[-1] + length $_ for @{$_[0]};
    return \@off;
}

sub load {
    my ($self, $ids, $seqs, $quals) = @_;
    die "Prgpu::Stages::load: ids, sequences and qualities differ in number\n" unless @$ids == @$seqs && @$seqs == @$quals;
    length $seqs->[$_] == length $quals->[$_] or die "Prgpu::Stages::load: $ids->[$_]: quality length != sequence length\n"
        for 0 .. $#$seqs;
    Prgpu::lrset_load($self->{h}, pack('q<*', @{_off($seqs)}), join('', @$seqs), join('', @$quals));
    $self->{ids} = [@$ids];
    return;
}

# the whole short-read input (nt4 pool, offsets as an array or packed int64) into HBM once
sub load_short_reads {
    my ($self, $pool, $off) = @_;
    Prgpu::srset_load($self->{h}, ref $off ? pack('q<*', @$off) : $off, $pool);
    return;
}

# One bwa-sr / bwa-mr task on the resident set.  ranges: the sample's record ranges
# [[first, last), ...]; sr_off: the sampled reads' offsets; params: the consensus options;
# bin_filter: [-b, -l] or undef; mask_cfg: [hcr-mask, min_sr_length] for the regular tasks,
# undef for the finish task (which maps to the unmasked reads).
sub task {
    my ($self, $task, $ranges, $sr_off, $params, $bin_filter, $mask_cfg) = @_;
    my $h = $self->{h};
    my $finish = !defined $mask_cfg;
    my @tp = (Time::HiRes::time());
    Prgpu::lrset_index($h, $finish ? READS : MAP);
    push @tp, Time::HiRes::time();
    my ($seed_opts, $sw_opts) = Prgpu::Tasks::options($task);
    @$sw_opts{qw(bin_size bin_length)} = (int($bin_filter->[0]), 0 + $bin_filter->[1]) if $bin_filter;
    my $status = Prgpu::seed_map_sampled($h, $seed_opts, pack('q<*', map { @$_ } @$ranges));
    die "Prgpu::Stages::task: the ranges hold " . length($status) / 4 . " short reads, the offsets $#$sr_off\n"
        unless length($status) / 4 == $#$sr_off;
    Prgpu::iter_upload_lrset($h, pack('q<*', @$sr_off));
    my %out = (n_tasks => Prgpu::seed_count($h), chim => [], bpt => 0, bpn => 0);
    push @tp, Time::HiRes::time();
    Prgpu::iter_launch($h, $sw_opts, $params);
    push @tp, Time::HiRes::time();
    if ($finish) {
        $out{chim} = [$self->_chim_lines];
    } else {
        $self->{stats} ||= Prgpu::dev_alloc($h, 16);   # the {bpt, bpN} device words, kept across tasks
        Prgpu::iter_mask($h, Prgpu::mask_params($mask_cfg->[0], $mask_cfg->[1]), $self->{stats});
        @out{qw(bpt bpn)} = unpack('q<2', Prgpu::dev_download($h, $self->{stats}, 16));
    }
    my @ms = Prgpu::stage_ms($h);
    my @names = qw(index seeding sw_extend sw_global_cigar exchange_handoff consensus);
    $self->{last_stage_ms} = {map { $names[$_] => sprintf('%.2f', $ms[$_]) + 0 } 0 .. $#names};
    $self->{device_ms} += $_ for @ms;
    push @tp, Time::HiRes::time();
    Prgpu::lrset_commit($h, $finish ? 0 : COMMIT_MASK);
    push @tp, Time::HiRes::time();
    # wall clock per part (ms, device work included), named as GpuStages names them
    my @parts = qw(index seed_sw_exchange consensus_launch chim_or_mask commit);
    $self->{last_part_ms} = {map { $parts[$_] => sprintf('%.2f', ($tp[$_ + 1] - $tp[$_]) * 1e3) + 0 } 0 .. $#parts};
    return \%out;
}

# bam2cns's chimera lines of every read of the last launch: "ID\tFROM\tTO\tRATIO" with the
# ratio in Perl's own number stringification, the reference's format
sub _chim_lines {
    my ($self) = @_;
    my $o = Prgpu::iter_chim($self->{h});
    my @nch = unpack('l<*', $o->{nchim});
    my @c0 = unpack('q<*', $o->{chim_off});
    my $ids = $self->{ids};
    my $n = @$ids < @nch ? @$ids : @nch;
    my @lines;
    for my $i (0 .. $n - 1) {
        next unless $nch[$i] > 0;
        my @c = unpack('l<*', substr($o->{chim}, 16 * $c0[$i], 16 * $nch[$i]));
        my $r = {id => $ids->[$i], chim => [map { [@c[4 * $_ .. 4 * $_ + 3]] } 0 .. $nch[$i] - 1]};
        push @lines, map { chomp(my $l = $_); $l } Prgpu::chim_lines($r);
    }
    return @lines;
}

sub _split {
    my ($pool, $off) = @_;
    return [map { substr($pool, $off->[$_], $off->[$_ + 1] - $off->[$_]) } 0 .. $#$off - 1];
}

# the current reads: (\@ids, \@seqs, \@quals)
sub reads {
    my ($self) = @_;
    my $d = Prgpu::lrset_download($self->{h}, 1, 1, 0);
    my @off = unpack('q<*', $d->{off});
    return ($self->{ids}, _split($d->{seq}, \@off), _split($d->{qual}, \@off));
}

# the mapping reference of the next task (LR.masked.fa), one string per read
sub masked {
    my ($self) = @_;
    my $d = Prgpu::lrset_download($self->{h}, 0, 0, 1);
    return _split($d->{map}, [unpack('q<*', $d->{off})]);
}

1;
