// Error reporting of a side library (libegs_mcmc.so, libegs_prune.so, libegs_feat.so): each keeps a last-error string of
// its own, apart from libegs_hip.so's.  Its one source file names the library, then includes this header:
//   #define EGS_SIDE_LIBRARY "egs_feat"
//   #include "egs_side_error.h"
//   extern "C" const char* egs_feat_last_error_string(void) { return egs_side::g_err; }
#pragma once
#include <stdio.h>
#include <string.h>

#include "egs_common.h"

namespace egs_side {

static thread_local char g_err[512] = "no error";

static void set_error(int code, const char* what, const char* file, int line) {
  const char* base = strrchr(file, '/');
  snprintf(g_err, sizeof(g_err), EGS_SIDE_LIBRARY " error %d: %s (%s:%d)", code, what ? what : "?",
           base ? base + 1 : file, line);
}

}  // namespace egs_side

#define SIDE_CHECK_ARG(cond)                                                              \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      ::egs_side::set_error(EGS_ERR_BAD_ARG, "bad argument: " #cond, __FILE__, __LINE__);  \
      return EGS_ERR_BAD_ARG;                                                             \
    }                                                                                     \
  } while (0)

#define SIDE_HIP(expr)                                                              \
  do {                                                                              \
    hipError_t e__ = (expr);                                                        \
    if (e__ != hipSuccess) {                                                        \
      ::egs_side::set_error((int)e__, hipGetErrorString(e__), __FILE__, __LINE__);   \
      return (int)e__;                                                              \
    }                                                                               \
  } while (0)
