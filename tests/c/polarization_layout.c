/* prints sizeof(rtgr_polarization) and the offsets of its members, as a C compiler lays them out (tests/test_polarization.py) */
#include <stddef.h>
#include <stdio.h>

#include "rtgr.h"

int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtgr_polarization), offsetof(rtgr_polarization, kind), offsetof(rtgr_polarization, flags),
           offsetof(rtgr_polarization, deg0), offsetof(rtgr_polarization, deg1), offsetof(rtgr_polarization, field),
           offsetof(rtgr_polarization, reserved));
    return 0;
}
