// build_id.cpp -- the library's identity (include/impc_qp.h): the version string with the git
// revision, and the build id, a hash the Makefile takes over every source of the library and the
// compiler flags.  The only unit that is rebuilt for every source change.
#include "../../include/impc_qp.h"

#ifndef IMPC_BUILD_ID  // set by the Makefile
#define IMPC_BUILD_ID "src-unknown"
#endif
#ifndef IMPC_GIT_REV
#define IMPC_GIT_REV "unknown"
#endif

const char *impc_version(void) { return "impc_qp 0.3.0 (OSQP 0.6.2 semantics, gfx950, git " IMPC_GIT_REV ")"; }
const char *impc_build_id(void) { return IMPC_BUILD_ID; }
