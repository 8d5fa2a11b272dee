// tokens_launch.h -- the name tokens_kernel.hip includes launch.h by; nothing is declared here.
#pragma once
#include "launch.h"
