package Prgpu::Tasks;

# proovread's per-task parameters for the Perl driver (bin/prgpu-proovread): the port of
# proovread_amd/tasks.py, which restates the proovread.cfg entries the sr / mr correction
# loop reads (mode-tasks, bwa-*, sr-coverage, hcr-mask, bin-size, detect-chimera) and the
# lookup rule of bin/proovread's cfg(KEY, TASK) (bin/proovread:1989-2024): a missing KEY
# loses a trailing `-<n>` (`bwa-mr-3` -> `bwa-mr`), and in a per-task hash the TASK's own
# entry, else the TASK without its counter, else DEF wins.
#
# bwa mem options become the option hashes Prgpu.xs parses (fill_seed_opts / fill_sw_opts)
# the way proovread_amd/bwa_proovread.py's parse_mem + options make pr_seed_opts /
# pr_sw_opts of them, so a task's options mean what `bwa-proovread mem` makes of them.
#
# The tables are package variables: bin/prgpu-proovread -c overlays them (overlay).

use strict;
use warnings;

our %MODE_TASKS = (
    'sr-noccs' => [qw(read-long bwa-sr-1 bwa-sr-2 bwa-sr-3 bwa-sr-4 bwa-sr-5 bwa-sr-6 bwa-sr-finish)],
    'mr-noccs' => [qw(read-long bwa-mr-1 bwa-mr-2 bwa-mr-3 bwa-mr-4 bwa-mr-5 bwa-mr-6 bwa-mr-finish)],
    # external alignments: listed so that -m names them; the driver refuses their tasks
    'sam' => [qw(read-long read-sam)],
    'bam' => [qw(read-long read-bam)],
);

# bwa mem option sets; a flag without a value stands alone
no warnings 'qw';   # -O 2,1 and its like are single words
our %BWA_OPTS = (
    'bwa-sr' => [qw(-a -Y -A 5 -B 11 -O 2,1 -E 4,3 -T 2.5 -k 12 -W 20 -w 40 -r 1 -D 0 -y 20 -L 30,30)],
    'bwa-sr-finish' => [qw(-a -Y -k 17 -W 18 -w 30 -r 1.5 -D .75 -A 5 -B 13 -O 15,19 -E 3,3 -T 4 -L 30,30)],
    'bwa-mr-1' => [qw(-a -Y -A 5 -B 11 -O 2,1 -E 4,3 -T 2.5 -k 12 -W 20 -w 40 -r 1 -D 0 -y 20 -L 30,30)],
    'bwa-mr' => [qw(-a -Y -k 13 -W 20 -w 40 -r 1 -D .5 -y 20 -A 5 -B 11 -O 2,1 -E 4,3 -T 3 -L 30,30)],
    'bwa-mr-finish' => [qw(-a -Y -k 19 -W 40 -w 30 -A 5 -B 13 -O 15,19 -E 3,3 -T 4 -L 30,30)],
);

our %SR_COVERAGE = (DEF => 15, 'bwa-sr-finish' => 30, 'bwa-mr-finish' => 30);
our %HCR_MASK = (DEF => '20,41,80,130,60,0.7',
                 map { $_ => '20,41,80,130,60,0.3' } qw(bwa-mr-4 bwa-mr-5 bwa-mr-6 bwa-sr-4 bwa-sr-5 bwa-sr-6));
our %BIN_SIZE = (DEF => 20, sr => 20, 'sr-noccs' => 20, mr => 50, 'mr-noccs' => 50, sam => 20, bam => 20);
# the reference lists read-sam but not read-bam: its quirk, kept
our %DETECT_CHIMERA = (DEF => 0, 'bwa-sr-finish' => 1, 'bwa-mr-finish' => 1, 'read-sam' => 1);

# loop-wide values (proovread.cfg: coverage-scale-factor, mask-shortcut-frac,
# mask-min-gain-frac; lr-min-length undef = twice the shortest short read)
our %LOOP = ('coverage-scale-factor' => 0.75, 'mask-shortcut-frac' => 0.92, 'mask-min-gain-frac' => 0.03,
             'lr-min-length' => undef);

sub _strip {
    my ($task) = @_;
    (my $t = $task) =~ s/-\d+$//;
    return $t;
}

# cfg(KEY) for a table of option sets: KEY, else KEY without its counter
sub cfg_key {
    my ($table, $key) = @_;
    return $table->{$key} if exists $table->{$key};
    return $table->{_strip($key)};
}

# cfg(KEY, TASK) of a per-task hash: the task, else the task without its counter, else DEF
sub cfg_task {
    my ($table, $task) = @_;
    return $table->{$task} if exists $table->{$task};
    return $table->{_strip($task)} if exists $table->{_strip($task)};
    return $table->{DEF};
}

# bin/proovread:636-642: `mr` beyond 150 bp short reads (noccs: no PacBio subreads)
sub mode_for { $_[0] > 150 ? 'mr-noccs' : 'sr-noccs' }

sub is_finish { $_[0] =~ /-finish$/ ? 1 : 0 }

sub bwa_argv {
    my ($task) = @_;
    my $opts = cfg_key(\%BWA_OPTS, $task);
    die "no bwa options for task $task\n" unless defined $opts;
    return @$opts;
}

# `bwa-proovread mem`'s own defaults (bwa_proovread.py parse_mem)
my %MEM_DEFAULT = (A => 1, B => 4, O => '6,6', E => '1,1', L => '5,5', T => 30, k => 19, W => 0, w => 100, r => 1.5,
                   D => 0.5, y => 20, c => 500, d => 100, t => 1, b => 0, l => 0);
my %MEM_FLAG = (a => 1, Y => 1, e => 1);

sub parse_mem {
    my (@argv) = @_;
    my %a = %MEM_DEFAULT;
    while (@argv) {
        my $x = shift @argv;
        my ($k) = $x =~ /^-([A-Za-z])$/ or die "bwa-proovread mem: unknown option '$x'\n";
        if ($MEM_FLAG{$k}) { $a{$k} = 1; next }
        die "bwa-proovread mem: unknown option '$x'\n" unless exists $MEM_DEFAULT{$k};
        die "bwa-proovread mem: option '$x' needs a value\n" unless @argv;
        $a{$k} = shift @argv;
    }
    return \%a;
}

sub _pair {
    my @v = map { 0 + $_ } split /,/, $_[0];
    return ($v[0], @v > 1 ? $v[1] : $v[0]);
}

# (seed_opts, sw_opts) of a bwa task: the hashes Prgpu.xs turns into pr_seed_opts /
# pr_sw_opts over the library's bwa-sr defaults, as bwa_proovread.options does
sub options {
    my ($task) = @_;
    my $a = parse_mem(bwa_argv($task));
    my ($o_del, $o_ins) = _pair($a->{O});
    my ($e_del, $e_ins) = _pair($a->{E});
    my ($clip5, $clip3) = _pair($a->{L});
    my %so = (finish => 0, min_seed_len => 0 + $a->{k}, w => 0 + $a->{w}, split_factor => 0 + $a->{r},
              max_mem_intv => 0 + $a->{y}, max_occ => 0 + $a->{c}, drop_ratio => 0 + $a->{D},
              # bwa: -W defaults to the minimum seed length
              min_chain_weight => $a->{W} > 0 ? 0 + $a->{W} : 0 + $a->{k},
              a => 0 + $a->{A}, o_del => $o_del, e_del => $e_del, o_ins => $o_ins, e_ins => $e_ins, b => 0 + $a->{B});
    my %wo = (finish => 0, a => 0 + $a->{A}, b => 0 + $a->{B}, o_del => $o_del, e_del => $e_del, o_ins => $o_ins,
              e_ins => $e_ins, w => 0 + $a->{w}, zdrop => 0 + $a->{d}, pen_clip5 => $clip5, pen_clip3 => $clip3,
              min_score_per_base => 0 + $a->{T},
              drop_ratio => 0 + $a->{D});   # mem_reg2sam drops secondaries below -D x their primary
    return (\%so, \%wo);
}

sub sr_coverage { 0 + cfg_task(\%SR_COVERAGE, $_[0]) }
sub hcr_mask { cfg_task(\%HCR_MASK, $_[0]) }
sub detect_chimera { cfg_task(\%DETECT_CHIMERA, $_[0]) ? 1 : 0 }
sub bin_size { int(cfg_task(\%BIN_SIZE, $_[0])) }

# A user configuration in proovread.cfg's own format (a Perl hash, read with `do`) over the
# tables: mode-tasks, sr-coverage, the loop-wide scalars and the bwa-* option sets (a string
# as on the command line or an array).  Other keys are ignored with one warning each.
sub overlay {
    my ($file) = @_;
    my $path = $file =~ m{^/} ? $file : "./$file";
    die "cannot read config $file: $!\n" unless -r $path;
    my @cfg = do $path;
    die "config $file: $@" if $@;
    my %cfg = @cfg == 1 && ref $cfg[0] eq 'HASH' ? %{$cfg[0]} : @cfg;
    for my $k (sort keys %cfg) {
        my $v = $cfg{$k};
        if ($k eq 'mode-tasks') {
            die "config $file: mode-tasks must be a hash of task lists\n" unless ref $v eq 'HASH';
            $MODE_TASKS{$_} = [@{$v->{$_}}] for keys %$v;
        } elsif ($k eq 'sr-coverage') {
            if (ref $v eq 'HASH') { $SR_COVERAGE{$_} = $v->{$_} for keys %$v }
            else { %SR_COVERAGE = (DEF => $v) }
        } elsif (exists $LOOP{$k}) {
            $LOOP{$k} = $v;
        } elsif ($k =~ /^bwa-/ && (ref $v eq 'ARRAY' || !ref $v)) {
            $BWA_OPTS{$k} = ref $v ? [@$v] : [split ' ', $v];
        } else {
            warn "prgpu-proovread: config key '$k' is not used by this driver\n";
        }
    }
    return;
}

1;
