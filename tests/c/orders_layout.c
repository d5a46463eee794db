/* prints sizeof(rtgr_disk_orders) and the offsets of its members, then the same of rtgr_order_planes, as a C compiler lays them out
   (tests/test_orders.py) */
#include <stddef.h>
#include <stdio.h>

#include "rtgr.h"

int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rtgr_disk_orders), offsetof(rtgr_disk_orders, max_order), offsetof(rtgr_disk_orders, flags),
           offsetof(rtgr_disk_orders, margin), offsetof(rtgr_disk_orders, transmission), offsetof(rtgr_disk_orders, pad));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtgr_order_planes), offsetof(rtgr_order_planes, count), offsetof(rtgr_order_planes, hit32),
           offsetof(rtgr_order_planes, state_end), offsetof(rtgr_order_planes, g), offsetof(rtgr_order_planes, rgb_order),
           offsetof(rtgr_order_planes, state0));
    return 0;
}
