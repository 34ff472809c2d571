/* mt_le.h -- little-endian reads of the host engines. */
#ifndef ZMT_MT_LE_H
#define ZMT_MT_LE_H

#include <stdint.h>

static inline uint32_t rd32(const uint8_t *p)
{
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static inline uint64_t rd64(const uint8_t *p)
{
	return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32;
}

#endif
