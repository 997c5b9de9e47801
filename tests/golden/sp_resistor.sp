* one port across a resistor: Y11 = 1/R (plus the gmin of the node), S11 = (1 - Z0/R) / (1 + Z0/R)
V1 a 0 DC 0 PORTNUM 1
R1 a 0 75
.SP DEC 2 1k 1meg
