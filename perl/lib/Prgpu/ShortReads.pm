package Prgpu::ShortReads;

# The short-read input as one byte stream (`cat` of the -s files) with its FASTQ / FASTA
# records, sampled per task like SeqChunker: the port of proovread_amd/correct.py's
# ShortReads and of the record parser and chunk selection of proovread_amd/seqchunker.py.
#
#   * with --chunk-number N the stream is cut into N chunks of ceil(bytes / N) bytes, and a
#     record belongs to the chunk its first byte falls into (the last chunk takes the rest);
#   * chunks are numbered from 1; the chunks of a task are F, F+1, ..., F+K-1 and the same K
#     chunks of every following step of --chunk-step chunks (Prgpu::Control's cov2seqchunker);
#   * the records' sequences are kept as one nt4 pool in stream order, so a task's sample is a
#     list of record ranges [first, last) -- what Prgpu::seed_map_sampled gathers on the device.
#
# Plain 4-line FASTQ is scanned natively (Prgpu::fastq4); FASTA, multi-line or irregular
# input goes through the record parser below.

use strict;
use warnings;
use Prgpu;

my $WS = qr/[ \t\n\r\x0b\x0c]/;

# (start, end) byte ranges of the FASTA / FASTQ records of a stream
sub records {
    my ($data) = @_;
    my $n = length $data;
    my $i = 0;
    ++$i while $i < $n && substr($data, $i, 1) =~ /[\r\n]/;
    return () if $i >= $n;
    my $first = substr($data, $i, 1);
    die "input is neither FASTA nor FASTQ\n" unless $first eq '>' || $first eq '@';
    my @rec;
    if ($first eq '>') {
        while ($i < $n) {
            my $j = index($data, "\n>", $i);
            my $end = $j < 0 ? $n : $j + 1;
            push @rec, [$i, $end];
            $i = $end;
        }
        return @rec;
    }
    while ($i < $n) {
        if (substr($data, $i, 1) =~ /[\r\n]/) { ++$i; next }
        my $p = $i;
        for (1 .. 4) {
            my $j = index($data, "\n", $p);
            $p = $j < 0 ? $n : $j + 1;
        }
        push @rec, [$i, $p];
        $i = $p;
    }
    return @rec;
}

# the sequence of one record: FASTA lines joined, FASTQ's second line; blanks stripped at the ends
sub _seq_of {
    my ($rec) = @_;
    my @l = split /\n/, $rec, -1;
    my $s;
    if (substr($rec, 0, 1) eq '>') {
        $s = join '', @l[1 .. $#l];
    } else {
        die "truncated FASTQ record\n" if @l < 2;
        $s = $l[1];
    }
    $s =~ s/^$WS+//;
    $s =~ s/$WS+$//;
    return $s;
}

# the chunk numbers SeqChunker writes
sub select_chunks {
    my ($n_chunks, $first, $step, $per_step, $last) = @_;
    $last = !defined $last || $last > $n_chunks ? $n_chunks : $last;
    ($step, $per_step) = ($n_chunks, $n_chunks) if $step <= 0;
    my $k0 = $first > 1 ? $first : 1;
    return grep { ($_ - $first) % $step < $per_step } $k0 .. $last;
}

sub new {
    my ($class, $data, $chunk_number) = @_;
    $chunk_number = 1000 unless defined $chunk_number;
    my $total = length $data;
    my (@starts, @off, $pool);
    my $rec = Prgpu::fastq4($data);
    if ($rec) {   # plain 4-line FASTQ: record starts, offsets and nt4 pool in one native pass
        @starts = unpack('q<*', $rec->{starts});
        @off = unpack('q<*', $rec->{off});
        $pool = $rec->{pool};
    } else {      # FASTA (multi-line) or irregular FASTQ: the record parser
        my @seqs;
        for my $r (records($data)) {
            push @starts, $r->[0];
            push @seqs, _seq_of(substr($data, $r->[0], $r->[1] - $r->[0]));
        }
        @off = (0);
        push @off, $off[-1] + length $_ for @seqs;
        $pool = Prgpu::nt4(join '', @seqs);
    }
    my $n_chunks = $chunk_number > 1 ? $chunk_number : 1;
    my @cnt = (0) x $n_chunks;
    {
        use integer;
        my $csize = $total ? ($total + $n_chunks - 1) / $n_chunks : 1;
        $csize = 1 if $csize < 1;
        for my $s (@starts) {
            my $c = $s / $csize;
            ++$cnt[$c < $n_chunks - 1 ? $c : $n_chunks - 1];
        }
    }
    # records of chunk k (1-based): [cfirst[k-1], cfirst[k])
    my @cfirst = (0);
    push @cfirst, $cfirst[-1] + $_ for @cnt;
    return bless {n_chunks => $n_chunks, cfirst => \@cfirst, off => \@off, pool => $pool, n => scalar @starts}, $class;
}

sub n { $_[0]{n} }

# the shortest record, or undef without records
sub min_length {
    my ($self) = @_;
    my $off = $self->{off};
    my $min;
    for my $i (1 .. $#$off) {
        my $l = $off->[$i] - $off->[$i - 1];
        $min = $l if !defined $min || $l < $min;
    }
    return $min;
}

# -> (record ranges [[first, last), ...] of the chunks SeqChunker writes for cov2seqchunker's
# parameters (undef: every record), the offsets of the sampled reads)
sub sample_ranges {
    my ($self, $sc) = @_;
    my $off = $self->{off};
    return ([[0, $self->{n}]], [@$off]) unless defined $sc;
    my $cf = $self->{cfirst};
    my @rg = grep { $_->[1] > $_->[0] } map { [$cf->[$_ - 1], $cf->[$_]] }
        select_chunks($self->{n_chunks}, $sc->{'--first-chunk'}, $sc->{'--chunk-step'}, $sc->{'--chunks-per-step'});
    my @so = (0);
    for my $r (@rg) {
        my $shift = $so[-1] - $off->[$r->[0]];
        push @so, map { $_ + $shift } @$off[$r->[0] + 1 .. $r->[1]];
    }
    return (\@rg, \@so);
}

1;
