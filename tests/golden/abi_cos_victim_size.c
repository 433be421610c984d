/* Prints sizeof(ksim_cos_victim) and its field offsets as the C compiler lays them out
 * (tests/test_desched_cos_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "ksim_engine.h"

int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ksim_cos_victim), offsetof(ksim_cos_victim, event),
           offsetof(ksim_cos_victim, node), offsetof(ksim_cos_victim, gpu_mask), offsetof(ksim_cos_victim, reserved),
           offsetof(ksim_cos_victim, gpu_left_milli), offsetof(ksim_cos_victim, similarity));
    return 0;
}
