// pr_last_error's text, set from any host file of the library (prgpu_api.cpp); no HIP here, so
// the host-only files (seed.cpp, bam_codec.cpp, trim.cpp) include this alone.  Both return `code`.
#pragma once
int set_error(int code, const char *fmt, ...);   // printf-style
int pr_set_error(int code, const char *msg);
