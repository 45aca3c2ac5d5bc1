package Prgpu::Loop;

# proovread's sr / mr correction loop for a Perl host (bin/prgpu-proovread): the port of
# proovread_amd/correct.py at world 1 -- read-long, per task SeqChunker sampling, the task on
# the device stages (Prgpu::Stages), the masked fraction and mask-shortcut-frac's splice of the
# task list, and the final outputs -- with the output path of proovread_amd/seqfilter.py
# (--substr, --trim-win, --min-length, --fasta) and proovread_amd/chimera_filter.py's
# conversion in-process: once the device context exists, nothing here starts a child process.
#
#   my $res = Prgpu::Loop::run(lr_records => [[$id, $seq, $qual_or_undef], ...],
#                              sr_data => $fastq_bytes, stages => $stages,
#                              cfg => {coverage => 50, sampling => 1, mode => undef});
#   Prgpu::Loop::write_outputs($res, $prefix);
#
# $res: {ids, seqs, quals, chim (the finish task's lines), ignored, log ([{task, n_sr, n_tasks,
# bpt, bpn, masked_frac, shortcut, wall_ms, pre_ms, stage_ms, part_ms}, ...])}.

use strict;
use warnings;
use Time::HiRes ();
use Prgpu;
use Prgpu::Tasks;
use Prgpu::Control;
use Prgpu::ShortReads;

my $WS = qr/[ \t\n\r\x0b\x0c]/;

sub _strip {
    my ($s) = @_;
    $s =~ s/^$WS+//;
    $s =~ s/$WS+$//;
    return $s;
}

sub slurp {
    my ($path) = @_;
    my $data;
    if ($path =~ /\.gz$/) {
        require IO::Uncompress::Gunzip;
        IO::Uncompress::Gunzip::gunzip($path => \$data, MultiStream => 1)
            or die "$path: $IO::Uncompress::Gunzip::GunzipError\n";
    } else {
        open my $fh, '<:raw', $path or die "$path: $!\n";
        local $/;
        $data = <$fh>;
        close $fh;
    }
    return defined $data ? $data : '';
}

# FASTA / FASTQ (optionally gzipped) -> [name (first word), sequence, quality (undef: FASTA)]
sub read_fastx {
    my ($path) = @_;
    my @l = split /\n/, slurp($path), -1;
    pop @l if @l && $l[-1] eq '';
    my $i = 0;
    ++$i while $i < @l && $l[$i] !~ /[^ \t\n\r\x0b\x0c]/;
    return () if $i >= @l;
    my @rec;
    if ($l[$i] =~ /^>/) {
        my ($name, @buf) = ($l[$i]);
        my $flush = sub { push @rec, [(split ' ', substr($name, 1))[0], join('', @buf), undef] };
        for my $ln (@l[$i + 1 .. $#l]) {
            if ($ln =~ /^>/) {
                $flush->();
                ($name, @buf) = ($ln);
            } else {
                push @buf, _strip($ln);
            }
        }
        $flush->();
    } elsif ($l[$i] =~ /^@/) {
        while ($i < @l) {
            if ($l[$i] !~ /[^ \t\n\r\x0b\x0c]/) { ++$i; next }
            my ($s, $q) = map { defined $_ ? _strip($_) : '' } @l[$i + 1, $i + 3];
            push @rec, [(split ' ', substr($l[$i], 1))[0], $s, $q];
            $i += 4;
        }
    } else {
        die "$path: neither FASTA nor FASTQ\n";
    }
    return @rec;
}

# ---------------------------------------------------------------------------- read-long

sub _num {
    return $_[0] =~ /^\s*([+-]?\d+(?:\.\d*)?)/ ? $1 * 1.0 : 0.0;
}

# bam2cns's `byfile` order: natural order over digit / non-digit runs
sub byfile_cmp {
    my ($x, $y) = @_;
    my @pa = split /(\d+)/, $x;
    my @pb = split /(\d+)/, $y;
    my $n = @pa > @pb ? @pa : @pb;
    for my $i (0 .. $n - 1) {
        return -1 if $i >= @pa;
        return 1 if $i >= @pb;
        my $r = $pa[$i] =~ /\d/ ? _num($pa[$i]) <=> _num($pb[$i]) : $pa[$i] cmp $pb[$i];
        return $r if $r;
    }
    return 0;
}

# read-long on [id, seq, qual or undef] records: FASTA reads get '$' qualities, reads shorter
# than stubby_length go to .ignored.tsv, sequences are upper-cased with every non-ACGTN
# character -> N, ids in `byfile` order.  -> (\@ids, \@seqs, \@quals, \@ignored)
sub read_long {
    my ($records, $stubby) = @_;
    my (%keep, @order, @ignored);
    for my $r (@$records) {
        my ($rid, $seq, $qual) = @$r;
        if (length($seq) < $stubby) {
            push @ignored, "$rid\tstubby";
            next;
        }
        die "Non-unique long read id ($rid)\n" if exists $keep{$rid};
        (my $s = $seq) =~ tr/acgtn/ACGTN/;
        $s =~ tr/ACGTN/N/c;
        $keep{$rid} = [$s, defined $qual ? $qual : '$' x length $s];
        push @order, $rid;
    }
    my @ids = sort { byfile_cmp($a, $b) } @order;
    return (\@ids, [map { $keep{$_}[0] } @ids], [map { $keep{$_}[1] } @ids], \@ignored);
}

# ---------------------------------------------------------------------------- the loop

sub _min { $_[0] < $_[1] ? $_[0] : $_[1] }

# tasks the device loop runs; anything else (ccs-1, blasr-utg, read-sam, ...) stays with
# proovread_amd.correct or the reference
sub check_tasks {
    for my $task (@_) {
        die "task $task is outside the sr / mr loops\n" unless $task =~ /^bwa-[sm]r/;
    }
}

sub run {
    my (%a) = @_;
    my %cfg = (coverage => 50, sampling => 1, %{$a{cfg} || {}});
    my $L = \%Prgpu::Tasks::LOOP;
    my $stages = $a{stages};
    my $t0 = Time::HiRes::time();
    my $srs = Prgpu::ShortReads->new($a{sr_data});
    my $min_sr = $cfg{min_sr_length} || ($srs->n ? $srs->min_length : 200);
    my $stubby = defined $cfg{lr_min_length} ? $cfg{lr_min_length}
               : defined $L->{'lr-min-length'} ? $L->{'lr-min-length'} : 2 * $min_sr;
    my $mode = $cfg{mode} || Prgpu::Tasks::mode_for($min_sr);
    my $list = $cfg{tasks} || $Prgpu::Tasks::MODE_TASKS{$mode} or die "unknown mode $mode\n";
    my @tasks = @$list;
    my ($ids, $seqs, $quals, $ignored) = ([], [], [], []);
    my @log;
    my $parse_ms = (Time::HiRes::time() - $t0) * 1e3;
    if (@tasks && $tasks[0] eq 'read-long') {
        ($ids, $seqs, $quals, $ignored) = read_long($a{lr_records}, $stubby);
        shift @tasks;
        check_tasks(@tasks);                  # before the first stage call
        $stages->load($ids, $seqs, $quals);   # the mapping reference starts as the reads
        $stages->load_short_reads($srs->{pool}, $srs->{off}) if $srs->n;
        push @log, {task => 'read-long', n_sr => 0, n_tasks => 0, bpt => 0, bpn => 0, shortcut => ''};
    } else {
        check_tasks(@tasks);
    }
    my ($chim, $tlog) = run_tasks($stages, $srs, \@tasks, \%cfg, $mode, $min_sr, scalar @$ids);
    push @log, @$tlog;
    ($ids, $seqs, $quals) = $stages->reads if @$ids;
    return {ids => $ids, seqs => $seqs, quals => $quals, chim => $chim, ignored => $ignored, log => \@log,
            sr_parse_ms => $parse_ms};
}

# The bwa-sr / bwa-mr tasks after read-long on the stages' resident long reads: per task
# SeqChunker sampling, the task on the stages, the {bpt, bpN} statistic and
# mask-shortcut-frac's splice of the task list.  -> (chimera lines of the finish task, a log
# entry per task)
sub run_tasks {
    my ($stages, $srs, $tasks, $cfg, $mode, $min_sr, $have_reads) = @_;
    my $L = \%Prgpu::Tasks::LOOP;
    my $sampler = Prgpu::Control::Sampler->new(sampling => $cfg->{sampling} ? 1 : 0);
    my (@fracs, @log, @chim);
    my $tc = 0;
    while ($tc < @$tasks) {   # the list may shrink: mask-shortcut-frac splices
        my $task = $tasks->[$tc];
        check_tasks($task);
        my $finish = Prgpu::Tasks::is_finish($task);
        my %ent = (task => $task, n_sr => 0, n_tasks => 0, bpt => 0, bpn => 0, shortcut => '');
        my $t_task = Time::HiRes::time();
        my $task_cov = Prgpu::Tasks::sr_coverage($task);
        my ($ranges, $sr_off) = $srs->sample_ranges($sampler->cov2seqchunker($cfg->{coverage}, $task_cov));
        $ent{n_sr} = $#$sr_off;
        my $cov = _min($cfg->{coverage}, $task_cov);
        my %params = (coverage => $cov * $L->{'coverage-scale-factor'}, bin_size => 20, trim => 1,
                      indel_taboo_length => 7, indel_taboo => 0.1, min_aln_length => 50, max_ins_length => 0,
                      fallback_phred => 1, phred_offset => 33, qv_offset => 33, use_ref_qual => $finish ? 0 : 1,
                      qual_weighted => 0, detect_chimera => $finish ? 1 : 0, invert_scores => 0);
        # bwa-proovread -b BIN -l BIN x min(cov, task cov)
        my $bsz = Prgpu::Tasks::bin_size($mode);
        $ent{pre_ms} = sprintf('%.2f', (Time::HiRes::time() - $t_task) * 1e3) + 0;
        my $r = $have_reads
            ? $stages->task($task, $ranges, $sr_off, \%params, [$bsz, $bsz * $cov],
                            $finish ? undef : [Prgpu::Tasks::hcr_mask($task), $min_sr])
            : {n_tasks => 0, chim => [], bpt => 0, bpn => 0};
        $ent{n_tasks} = $r->{n_tasks};
        push @chim, @{$r->{chim}};
        unless ($finish) {
            @ent{qw(bpt bpn)} = @$r{qw(bpt bpn)};
            $ent{masked_frac} = $r->{bpt} ? Prgpu::Control::masked_fraction($r->{bpt}, $r->{bpn}) : 0.0;
            $ent{shortcut} = Prgpu::Control::mask_shortcut($tasks, $tc, $ent{masked_frac}, \@fracs,
                                                           $L->{'mask-shortcut-frac'}, $L->{'mask-min-gain-frac'});
        }
        $ent{wall_ms} = sprintf('%.1f', (Time::HiRes::time() - $t_task) * 1e3) + 0;
        if ($have_reads) {
            $ent{stage_ms} = $stages->{last_stage_ms};
            $ent{part_ms} = $stages->{last_part_ms};
        }
        push @log, \%ent;
        ++$tc;
    }
    return (\@chim, \@log);
}

# ---------------------------------------------------------------------------- outputs

# a number as Perl reads a string's leading number (chimera_filter.py's _perl_num)
sub _score {
    my ($s) = @_;
    return defined $s && $s =~ /^\s*([+-]?(?:\d+\.?\d*(?:[eE][+-]?\d+)?|\.\d+(?:[eE][+-]?\d+)?))/ ? $1 + 0 : 0;
}

# bam2cns chimera annotations -> SeqFilter --substr coordinates, as chimera_filter.convert
# restates ChimeraToSeqFilter with its behaviour on real input: the first line is a header;
# the first line of every read only opens the read; a read's pieces are written when the next
# id starts, so the last read of the file never is.
sub chimera_convert {
    my ($lines, $min_score) = @_;
    $min_score = 0.01 unless defined $min_score;
    my @out;
    my ($rid, @coords) = ('');
    for my $k (1 .. $#$lines) {
        (my $raw = $lines->[$k]) =~ s/\n+$//;
        my @f = split /\t/, $raw, -1;
        pop @f while @f && $f[-1] eq '';
        my $id = @f ? $f[0] : '';
        if ($id ne $rid) {
            if (@coords) {
                my @c = ('0', @coords);
                my $i = 0;
                for (; $i < $#c; $i += 2) { push @out, "$rid\t$c[$i]\t$c[$i + 1]" }
                push @out, "$rid\t$c[$i]";
            }
            ($rid, @coords) = ($id);
        } elsif (_score($f[3]) >= $min_score) {
            push @coords, (defined $f[1] ? $f[1] : ''), (defined $f[2] ? $f[2] : '');
        }
    }
    return @out;
}

# FASTQ records of a file as seqfilter.read_records reads them: [id, description, seq, qual]
sub read_records {
    my ($path) = @_;
    my @l = split /\n/, slurp($path), -1;
    my $i = 0;
    ++$i while $i < @l && $l[$i] !~ /[^ \t\n\r\x0b\x0c]/;
    return () if $i >= @l;
    die "$path: FASTQ expected\n" unless $l[$i] =~ /^@/;
    my @rec;
    while ($i < @l) {
        if ($l[$i] !~ /[^ \t\n\r\x0b\x0c]/) { ++$i; next }
        die "$path: truncated or malformed FASTQ record at line " . ($i + 1) . "\n" if $i + 3 >= @l || $l[$i] !~ /^@/;
        (my $head = substr($l[$i], 1)) =~ s/\r+$//;
        my ($seq, $qual) = (_strip($l[$i + 1]), _strip($l[$i + 3]));
        die "$path: record '" . substr($head, 0, 40) . "': quality length != sequence length\n"
            if length $seq != length $qual;
        my ($rid, $desc) = split ' ', $head, 2;
        push @rec, [defined $rid ? $rid : '', defined $desc ? $desc : '', $seq, $qual];
        $i += 4;
    }
    return @rec;
}

sub format_fastq {
    my ($r) = @_;
    my $head = $r->[0] . (length $r->[1] ? " $r->[1]" : '');
    return "\@$head\n$r->[2]\n+\n$r->[3]\n";
}

sub format_fasta {
    my ($r, $width) = @_;
    my $head = $r->[0] . (length $r->[1] ? " $r->[1]" : '');
    my @out = (">$head");
    if ($width && $width > 0) {
        for (my $k = 0; $k < length $r->[2]; $k += $width) { push @out, substr($r->[2], $k, $width) }
    } elsif (length $r->[2]) {
        push @out, $r->[2];
    }
    return join("\n", @out) . "\n";
}

# --substr lines `id start end` or `id start` (to the read end) -> {id => [[start, end or undef]]}
sub parse_substr {
    my %d;
    for my $ln (@_) {
        (my $l = $ln) =~ s/\n+$//;
        my @f = split /\t/, $l, -1;
        next if @f < 2 || $f[0] eq '';
        push @{$d{$f[0]}}, [int($f[1]), @f > 2 && $f[2] ne '' ? int($f[2]) : undef];
    }
    return \%d;
}

sub _pieces {
    my ($len, $ranges) = @_;
    my @out;
    for my $r (@$ranges) {
        my ($s, $e) = @$r;
        $e = !defined $e || $e > $len ? $len : $e;
        $s = $s > $len ? $len : $s;
        $s = 0 if $s < 0;
        push @out, [$s, $e - $s > 0 ? $e - $s : 0];
    }
    return \@out;
}

# the (offset, length) pieces of a record: one piece keeps the id, several become id.1, id.2 ...;
# descriptions gain SUBSTR:offset,length
sub _split_rec {
    my ($r, $ranges) = @_;
    my ($rid, $desc, $seq, $qual) = @$r;
    my $many = @$ranges > 1;
    my ($k, @res) = (0);
    for my $p (@$ranges) {
        ++$k;
        my ($o, $l) = @$p;
        my $tag = "SUBSTR:$o,$l";
        push @res, [$many ? "$rid.$k" : $rid, length $desc ? "$desc $tag" : $tag,
                    $o < length $seq ? substr($seq, $o, $l) : '', $o < length $qual ? substr($qual, $o, $l) : ''];
    }
    return @res;
}

# `SeqFilter --trim-win W --min-length N --substr SUBSTR --phred-offset 33` on records
sub trim_records {
    my ($recs, $substr_lines, $trim_win, $min_length, $threads) = @_;
    my $sub = parse_substr(@$substr_lines);
    my @recs = map { exists $sub->{$_->[0]} ? _split_rec($_, _pieces(length $_->[2], $sub->{$_->[0]})) : $_ } @$recs;
    my $p = Prgpu::trim_params($trim_win);
    $p->{phred_offset} = 33;
    my @off = (0);
    push @off, $off[-1] + length $_->[3] for @recs;
    my $w = Prgpu::trim_windows($p, join('', map { $_->[3] } @recs), pack('q<*', @off), $threads || 0);
    my @woff = unpack('q<*', $w->{win_off});
    my @nw = unpack('l<*', $w->{n_win});
    my @out;
    for my $i (0 .. $#recs) {
        next unless $nw[$i];
        my @v = unpack('l<*', substr($w->{win}, 8 * $woff[$i], 8 * $nw[$i]));
        push @out, _split_rec($recs[$i], [map { [@v[2 * $_, 2 * $_ + 1]] } 0 .. $nw[$i] - 1]);
    }
    return grep { length $_->[2] >= $min_length } @out if $min_length;
    return @out;
}

sub _write {
    my ($path, $text) = @_;
    open my $fh, '>:raw', $path or die "$path: $!\n";
    print $fh $text;
    close $fh or die "$path: $!\n";
}

# The files of the job's end: PRE.untrimmed.fq, PRE.chim.tsv (the finish task's chimera lines
# as --substr coordinates), PRE.ignored.tsv, PRE.trimmed.fq (--trim-win 12,5 --min-length 500
# --substr PRE.chim.tsv) and, when that is not empty, PRE.trimmed.fa.  Options: min_length,
# trim_win, threads (the trim windows' host threads; 0: all cores).
sub write_outputs {
    my ($res, $pre, %o) = @_;
    my $min_length = defined $o{min_length} ? $o{min_length} : 500;
    my $trim_win = defined $o{trim_win} ? $o{trim_win} : '12,5';
    my ($ids, $seqs, $quals) = @$res{qw(ids seqs quals)};
    _write("$pre.untrimmed.fq", join('', map { "\@$ids->[$_]\n$seqs->[$_]\n+\n$quals->[$_]\n" } 0 .. $#$ids));
    my @sub = chimera_convert(["#id\tfrom\tto\tscore", @{$res->{chim}}]);   # correct_sr_mt's header
    _write("$pre.chim.tsv", join('', map { "$_\n" } @sub));
    _write("$pre.ignored.tsv", join('', map { "$_\n" } @{$res->{ignored}}));
    my @trimmed = trim_records([read_records("$pre.untrimmed.fq")], \@sub, $trim_win, $min_length, $o{threads});
    my $fq = join '', map { format_fastq($_) } @trimmed;
    _write("$pre.trimmed.fq", $fq);
    _write("$pre.trimmed.fa", join '', map { format_fasta($_, 80) } read_records("$pre.trimmed.fq")) if length $fq;
    return;
}

# PRE.tasks.tsv: one row per task
sub write_task_log {
    my ($res, $path) = @_;
    my $text = "#task\tn_sr\tn_seeds\tbpt\tbpN\tmasked_frac\tshortcut\n";
    for my $e (@{$res->{log}}) {
        $text .= join("\t", @$e{qw(task n_sr n_tasks bpt bpn)}, defined $e->{masked_frac} ? $e->{masked_frac} : '',
                      $e->{shortcut}) . "\n";
    }
    _write($path, $text);
}

1;
