/* Prints sizeof(ksim_victim) and its field offsets as the C compiler lays them out (tests/test_desched_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "ksim_engine.h"

int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ksim_victim), offsetof(ksim_victim, event),
           offsetof(ksim_victim, node), offsetof(ksim_victim, gpu_mask), offsetof(ksim_victim, score),
           offsetof(ksim_victim, frag_before), offsetof(ksim_victim, frag_after));
    return 0;
}
