#!/bin/sh
# Regenerates the ccs-1 golden fixtures from the reference Perl engine.
# Needs the reference checkout (PROOVREAD_REFERENCE) and the built library; outputs are committed.
set -e
cd "$(dirname "$0")"
python3 make_ccs_cases.py ccs_cases.txt
PERL_HASH_SEED=0 PERL_PERTURB_KEYS=0 perl gen_ccs_golden.pl ccs_cases.txt > ccs_expected.txt
