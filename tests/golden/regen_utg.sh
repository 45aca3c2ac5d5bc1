#!/bin/sh
# Regenerates the unitig consensus golden fixtures from the reference Perl engine.
# Needs the reference checkout (PROOVREAD_REFERENCE).  The reference walks Perl hashes; the
# fixture is written only if three hash seeds give the same bytes, and their digests go into its
# header.  PERL_HASH_SEED_DEBUG must be unset.
set -e
cd "$(dirname "$0")"
unset PERL_HASH_SEED_DEBUG
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
python3 make_utg_cases.py "$tmp/utg_cases.txt"
for seed in 0 17 4242; do
    PERL_HASH_SEED=$seed PERL_PERTURB_KEYS=2 perl gen_utg_golden.pl "$tmp/utg_cases.txt" > "$tmp/$seed.txt"
done
cmp "$tmp/0.txt" "$tmp/17.txt"
cmp "$tmp/0.txt" "$tmp/4242.txt"
{
    echo "# unitig consensus: the reference's results for utg_cases.txt.gz (gen_utg_golden.pl)"
    for seed in 0 17 4242; do
        echo "# PERL_HASH_SEED=$seed sha256 $(sha256sum < "$tmp/$seed.txt" | cut -d' ' -f1)"
    done
    cat "$tmp/0.txt"
} > utg_expected.txt
# the inputs are generated data (make_utg_cases.py): kept compressed, without a time stamp
gzip -n -9 -c "$tmp/utg_cases.txt" > utg_cases.txt.gz
