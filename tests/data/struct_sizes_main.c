/* Prints the size and the field offsets of the C ABI's reduction structs as a C compiler lays them out
 * (tests/test_reduce_host.py compares them with the ctypes mirror in lorastencil_amd/_lib.py). */
#include <stddef.h>
#include <stdio.h>

#include "lorastencil.h"

#define SIZE(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
    SIZE(lora_grid_stats);
    OFF(lora_grid_stats, abs_max);
    OFF(lora_grid_stats, count);
    OFF(lora_grid_stats, nonfinite);
    SIZE(lora_grid_diff);
    OFF(lora_grid_diff, argmax);
    OFF(lora_grid_diff, nonfinite);
    SIZE(lora_until);
    OFF(lora_until, norm);
    OFF(lora_until, max_times);
    SIZE(lora_until_result);
    OFF(lora_until_result, residual);
    OFF(lora_until_result, last);
    return 0;
}
