package Prgpu::Control;

# Iteration control around the hot path (the port of proovread_amd/control.py):
#
#   Sampler->cov2seqchunker  short-read sampling per iteration (bin/proovread:2085-2102):
#                            which SeqChunker chunks feed the next task;
#   mask_shortcut            the skip rule on the masked fraction bpN/bpt
#                            (bin/proovread:2026-2047), splicing the task list;
#   masked_fraction          bpN/bpt of the masking statistic (bin/proovread:1711-1716).

use strict;
use warnings;

package Prgpu::Control::Sampler;

# the `$first_chunk` global of proovread and the cfg values it uses (sr-chunk-number,
# sr-chunk-step); sampling => 0 is --no-sampling
sub new {
    my ($class, %a) = @_;
    return bless {chunk_number => 1000, chunk_step => 20, first_chunk => 1, sampling => 1, %a}, $class;
}

# SeqChunker parameters for sr coverage c and target tc, or undef (no sampling)
sub cov2seqchunker {
    my ($self, $c, $tc) = @_;
    return undef unless $self->{sampling};
    return undef if $c * 0.8 < $tc;   # don't sample if the target is more than 80 % of the data
    my $per_step = int($self->{chunk_step} * ($tc / $c) + .5);
    my %sc = ('--chunk-number' => $self->{chunk_number}, '--chunk-step' => $self->{chunk_step},
              '--chunks-per-step' => $per_step, '--first-chunk' => $self->{first_chunk});
    $self->{first_chunk} += $per_step;
    $self->{first_chunk} -= $self->{chunk_step} if $self->{first_chunk} > $self->{chunk_step};
    return \%sc;
}

package Prgpu::Control;

sub masked_fraction {
    my ($bpt, $bpn) = @_;
    return $bpn / $bpt;   # proovread divides unguarded
}

# bin/proovread:2026-2047 on the task list (edited in place like @TASKS).  Returns "skip" (all
# but the last task dropped: masked > shortcut_frac, or the gain over the previous iteration
# < min_gain), "continue", or "" when the check does not apply (no shortcut fraction, or tc is
# the second-to-last task or later).
sub mask_shortcut {
    my ($tasks, $tc, $masked_frac, $fracs, $shortcut_frac, $min_gain) = @_;
    $shortcut_frac = 0.92 unless defined $shortcut_frac;
    $min_gain = 0.03 unless defined $min_gain;
    return '' if !$shortcut_frac || $tc >= @$tasks - 2;
    my $prev = @$fracs ? $fracs->[-1] : -$min_gain;
    my $res = 'continue';
    if ($masked_frac > $shortcut_frac) {
        $res = 'skip';
    } elsif ($prev && ($masked_frac - $min_gain) < $prev) {
        $res = 'skip';
    }
    splice(@$tasks, $tc + 1, @$tasks - $tc - 2) if $res eq 'skip';   # every task between tc and the last
    push @$fracs, $masked_frac;
    return $res;
}

1;
