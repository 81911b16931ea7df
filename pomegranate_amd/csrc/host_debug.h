/* host_debug.h -- the debug switches of POM_LZO_DEBUG ("key=value,...";
 * host_debug.c).  Internal to liblzo_mi355x.so; plain C, no HIP. */
#ifndef POM_HOST_DEBUG_H
#define POM_HOST_DEBUG_H 1

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The value of `key` copied into buf (cut to n - 1 bytes), or NULL when the
 * key is absent. */
const char *pom_dbg_str(const char *key, char *buf, size_t n);
/* Its integer value; dflt when the key is absent or empty. */
long pom_dbg_int(const char *key, long dflt);

#ifdef __cplusplus
}
#endif

#endif
