// What bam_codec.cpp (host only, no HIP) offers the library's other host files; ctx.h includes it.
#pragma once
// Perl's numification of an AS:Z string: optional spaces, then a number, else 0 (AS:Z scores)
double bam_perl_number(const char *s, const char *e);
